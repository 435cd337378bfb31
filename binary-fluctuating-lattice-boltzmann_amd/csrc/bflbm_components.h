// bflbm_components.h -- component traces: per connected component of the set {v >= level} or {v < level} of one observed
// hydrovs or hydrovsbar variable (the cluster trace's components and labels, bflbm_cluster.h) its size, a periodic-safe
// origin, its extent along every axis, the first and second integer moments of its sites about that origin and its
// area in cell faces, for the `rows` qualifying components of smallest label, recorded on the device as 64-bit integers
// for a lone single-slab context or every replica of a batch (include/bflbm.h, "Component traces": the definition and the
// layout of a sample are stated there and only there).  Without this a user downloads the labels per sample
// (bflbm_cluster_labels, 4 bytes per site) and sums on the host; the ensemble trace's one centre of mass means nothing
// with two droplets in the box.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   of the one variable, exactly as the cluster trace takes it (fields_observe),
//   per level, one after another through the same arrays parent and size, int32 [replica][nsites]:
//   cluster_label_level             k_cluster_local and k_cluster_merge, and
//   cluster_resolve_level           k_cluster_resolve: the cluster trace's launches, called and not copied.  Afterwards a
//                                   site reaches its global root in two plain loads: a = parent[p] is its brick-local root
//                                   (p itself where p is one), parent[a] the global root (a itself where a is one).
//   k_component_count               1024 sites per workgroup: header words 0..3 summed per wave and workgroup, one 64-bit
//                                   global add per non-zero word and workgroup; the workgroup's number of qualifying roots
//                                   (parent[p] == p, size[p] >= min_size) into counts[replica][workgroup].
//   k_component_scan                one workgroup per replica: counts become their exclusive prefix sums, 256 at a time.
//   k_component_rank                the count launch's workgroups again: a qualifying root's rank is its workgroup's prefix
//                                   plus the qualifying roots before it in the workgroup (wave ballots, 16 wave counts in
//                                   LDS): the number of qualifying roots of smaller index, whatever the launch geometry.
//                                   Label and size go into row `rank` where rank < rows; size[root] becomes the root's
//                                   slot (the rank, or -1: not qualifying or not tabulated).  Sizes are not read again.
//   k_component_masks               one workgroup per brick of 32 x 4 x 4 (k_cluster_local's): per key (below) the brick's
//                                   32 + 4 + 4 coordinate bits by 32-bit LDS atomic ORs, then one 64-bit global atomic OR
//                                   per (key present, axis) into masks[replica][slot][axis][bits]: a brick's bits of an
//                                   axis lie in one 64-bit word because 64 is a multiple of every brick extent.
//   k_component_origin              one thread per (replica, slot, axis): component_arc turns the mask into origin and
//                                   extent, written into the row, and clears the mask for the next level.
//   k_component_moments             one workgroup per brick: per key the 9 sums and the faces in LDS by 64-bit LDS atomic
//                                   adds (one add per wave and word where a wave's occupied sites share one key), then one
//                                   64-bit global add per (key present, non-zero word) into the row.
//   and once, k_component_finish    header and rows of all levels into the slot, word 4 and the unused rows' label -1
//                                   formed, the staging cleared.
// The phases are separated by launches, not by a grid barrier: a stuck barrier is a hang.
// Key: within a brick, the sites of one brick-local component must meet in one LDS accumulator without a search.  The key
// of an occupied site p is the brick-local index of a = parent[p] where a lies in p's brick, else p's own (then p is a
// brick-local root whose global root lies elsewhere).  a lies in p's brick for every site that is not a brick-local root
// (k_cluster_local wrote it, and merge and resolve re-point roots only) and otherwise only where the global root does:
// either way the key is a site of this brick in p's component, and all sites of a brick-local component share it.  Two keys
// of one component in one brick cost a second flush, nothing else.  As in k_cluster_resolve the global atomics per
// component are then the bricks it touches (times 3 mask words, times at most 10 sums), not its sites.
// Arc: neighbouring sites differ by at most 1 per coordinate, modulo the extent, under either connectivity, so the
// projection of a connected component on an axis is connected on the periodic axis: one arc, or all of it.  An arc has
// exactly one occupied coordinate whose predecessor is unoccupied: the origin.  d_a = (c_a - o_a) mod n_a then unwraps a
// non-spanning axis wherever the component lies across the periodic planes.  Spanning (extent_a == n_a) is necessary for
// wrapping, not sufficient: a path may cover every x without a link across the x plane.
// Faces: a component's count of (site, one of 6 directions) with an unoccupied periodic neighbour.  Summed over all
// components, every occupied site counts its unoccupied neighbours: sum = 6 N3 - #(ordered pairs of occupied sites along
// an axis direction).  Per axis and site x, [o(x) | o(x+)] = o(x) + o(x+) - o(x) o(x+), so N2 = 3 N3 + 3 N3 - P with P the
// unordered occupied pairs (x, x+), and the ordered pairs are 2 P = 12 N3 - 2 N2: sum = -6 N3 + 2 N2 = S, the morphology
// trace's area, on extents 1 and 2 as well (the neighbour is the site itself, or counts twice).
// Overflow: extents above 65536 are refused, so d_a d_b < 2^32; nsites <= 2^31 - 1 gives every sum of a component
// < 2^31 2^32 = 2^63 (for a != b, d_a d_b < n_a n_b <= nsites, far less).  A brick has 512 sites: an LDS accumulator
// holds less than 2^9 2^32 = 2^41, which no 32-bit word does; hence 64-bit LDS atomics.  Faces: at most 6 per site.  The
// only 32-bit counters are counts of sites or roots of one workgroup (<= 1024) and the scan's prefix (< 2^31 roots).
// Coherence: no kernel here reads what another workgroup of the same launch writes.  The global writes inside a launch
// are relaxed agent-scope atomic read-modify-writes (OR, add) performed at the point of coherence and never read back in
// that launch, or plain stores to words only that thread owns (a root's slot, a row's label and size, an origin).  What
// a later launch reads (parents, slots, origins, the sums) is ordered by the launch boundary: plain loads.  No loop here
// follows parents: the two loads above need none.  The loops of the three labelling launches carry the cluster trace's
// cap and count into header word 5.  A slot read from a defective labelling is range-checked before it indexes anything.
// Memory per site and replica: parent and size, 8 bytes; a batch also the dense field, 8 bytes.  Besides: per replica
// rows x ((nx + 63) / 64 + (ny + 63) / 64 + (nz + 63) / 64) mask words and 4 bytes per 1024 sites of counts.
// Expected traffic per site and level, derived, not measured: the cluster trace's labelling (about 24 bytes: local 16, merge
// 4, resolve 4); count 8 (parent, and size at the roots); rank 4 + 4; masks 4 (parent) plus parent[a] and the slot, which a
// brick's sites share through the caches; moments 4 plus the same, the 6 neighbours' parents (re-loads of lines the brick
// and its 6 neighbours own) and 24 bytes of origin per wave: about 50 bytes against the 608 of a step.
// Out of scope: mass-weighted or second-variable sums per component (a float sum per component has no fixed order under
// atomics), true wrapping (winding) detection, tracking on the device (analysis.track_components links rows on the
// host), rings, 18-connectivity.
// Host part: plain C++17 on top of bflbm_cluster.h's.  A stand-alone program defines BFLBM_COMPONENTS_HOST_ONLY (and the
// CLUSTER, MORPH and FIELDSEL ones) and includes it after bflbm_cluster.h.  Included by bflbm.hip after bflbm_cluster.h.
#ifndef BFLBM_COMPONENTS_H_
#define BFLBM_COMPONENTS_H_

namespace component_limits {
constexpr int kHeader = 6;                       // ncomp, V, nqual, Vqual, nrows, capped
constexpr int kRowWords = 18;
constexpr int kMaxRows = 256;
constexpr int kLabel = 0, kSize = 1, kOrigin = 2, kExtent = 5, kSum = 8, kSum2 = 11, kCross = 14, kFaces = 17;
constexpr int kSums = 10;                        // the words a brick accumulates in LDS: 8 .. 17
constexpr int kCapped = 5;                       // the header word that counts loops that hit their cap
constexpr int kRankSites = 4 * cluster_limits::kThreads;   // sites of a workgroup of k_component_count and k_component_rank
constexpr int kLaunches = 9;                     // per level: local, merge, resolve, count, scan, rank, masks, origin, moments
constexpr int kMaxExtent = 65536;                // d_a d_b < 2^32
static_assert(kSum + kSums == kRowWords && kFaces == kRowWords - 1, "the sums end the row");
static_assert(64 % cluster_limits::kBx == 0 && 64 % cluster_limits::kBy == 0 && 64 % cluster_limits::kBz == 0, "a brick's bits of an axis lie in one word");
}

// the 64-bit words of a level's record, of an axis' mask and of a slot's three masks
BFLBM_CLUSTER_FN long long component_words(int rows) { return component_limits::kHeader + (long long)rows * component_limits::kRowWords; }
BFLBM_CLUSTER_FN int component_mask_words(int n) { return (n + 63) / 64; }
BFLBM_CLUSTER_FN int component_slot_words(const ClusterBox& B) { return component_mask_words(B.nx) + component_mask_words(B.ny) + component_mask_words(B.nz); }

// Origin and extent of the occupied coordinates of a periodic axis of n sites, bit c of w[c / 64] (bits >= n are zero): the
// extent is their number; the origin the occupied coordinate whose predecessor (c - 1) mod n is unoccupied, the smallest
// if a defect left more than one, and 0 where none has one: an empty mask or a spanned axis.
BFLBM_CLUSTER_FN void component_arc(const unsigned long long* w, int n, long long* origin, long long* extent) {
  const int nw = component_mask_words(n);
  unsigned long long carry = (w[(n - 1) >> 6] >> ((n - 1) & 63)) & 1ull;      // the predecessor of coordinate 0 is n - 1
  long long o = 0, e = 0;
  bool found = false;
  for (int i = 0; i < nw; ++i) {
    const unsigned long long b = w[i];
    e += __builtin_popcountll(b);
    const unsigned long long starts = b & ~((b << 1) | carry);
    if (!found && starts) { o = (long long)i * 64 + __builtin_ctzll(starts); found = true; }
    carry = b >> 63;
  }
  *origin = o; *extent = e;
}

// d = (c - o) mod n for 0 <= c, o < n
BFLBM_CLUSTER_FN int component_offset(int c, int o, int n) { return c >= o ? c - o : c - o + n; }

// The key of an occupied site whose parent is the site a, in the brick at (x0, y0, z0): a's brick-local index where a
// lies in the brick, else -1 (the caller then takes the site's own).
BFLBM_CLUSTER_FN int component_key(const ClusterBox& B, int x0, int y0, int z0, int a) {
  using namespace cluster_limits;
  const int za = a / (B.nx * B.ny), ya = (a - za * B.nx * B.ny) / B.nx, xa = a - (za * B.ny + ya) * B.nx;
  const int lx = xa - x0, ly = ya - y0, lz = za - z0;
  if (lx < 0 || lx >= kBx || ly < 0 || ly >= kBy || lz < 0 || lz >= kBz) return -1;
  return (lz * kBy + ly) * kBx + lx;
}

// the periodic neighbour of coordinate c along direction d = -1 or +1 on an axis of n sites (an extent of 1: itself)
BFLBM_CLUSTER_FN int component_wrap(int c, int d, int n) { const int t = c + d; return t < 0 ? t + n : (t >= n ? t - n : t); }

namespace {

// What every creation call refuses about its arguments: the cluster trace's refusals in its order, then min_size and rows.
int component_refuse_args(const char* call, int source, int var, int nlevels, const double* levels, int side, int connectivity, long long min_size,
                          int rows) {
  if (cluster_refuse_args(call, source, var, nlevels, levels, side, connectivity)) return 1;
  if (min_size < 1) return fail("%s: min_size must be >= 1 (got %lld)", call, min_size);
  if (rows < 1 || rows > component_limits::kMaxRows) return fail("%s: rows must be in 1..%d (got %d)", call, component_limits::kMaxRows, rows);
  return 0;
}
// the cluster trace's site limit, then the extents: the second moments are argued for d_a d_b < 2^32
int component_refuse_sites(const char* call, int nx, int ny, int nz) {
  if (cluster_refuse_sites(call, nx, ny, nz)) return 1;
  const int longest = std::max(nx, std::max(ny, nz));
  if (longest > component_limits::kMaxExtent)
    return fail("%s: an extent of %d exceeds %d (the second moments are 64-bit)", call, longest, component_limits::kMaxExtent);
  return 0;
}

inline long long component_groups(long long nsites) { return (nsites + component_limits::kRankSites - 1) / component_limits::kRankSites; }

}  // namespace

#ifndef BFLBM_COMPONENTS_HOST_ONLY

// d_rec [capacity][nrep][nlevels][6 + rows 18] as long long, d_stage: the same words of one sample, summed into
struct bflbm_component : bflbm_sample_store {
  ClusterBox B;
  long long nsites = 0, min_size = 1;
  int rows = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar; one variable
  MorphLevels L;
  double* fields = nullptr;         // a batch: [nrep][nsites]
  int* parent = nullptr;            // [nrep][nsites]
  int* size = nullptr;              // [nrep][nsites]; after k_component_rank a global root's word is its slot
  unsigned long long* masks = nullptr;   // [nrep][rows][slot words]; zero between the levels
  unsigned* counts = nullptr;       // [nrep][groups]
  bflbm_component() : bflbm_sample_store("component trace", "bflbm_component") {}
  ~bflbm_component() override {
    if (!fields && !parent && !size && !masks && !counts) return;
    hipSetDevice(device);
    if (fields) hipFree(fields);
    if (parent) hipFree(parent);
    if (size) hipFree(size);
    if (masks) hipFree(masks);
    if (counts) hipFree(counts);
  }
  unsigned long long* totals() const { return reinterpret_cast<unsigned long long*>(d_stage); }
  size_t words() const { return (size_t)nrep * L.n * (size_t)component_words(rows); }
  size_t mask_words() const { return (size_t)nrep * rows * (size_t)component_slot_words(B); }
  ClusterArrays arrays() const { return ClusterArrays{recorder_stream(this), nrep, nsites, B, parent, size}; }
  int record() override;
};

namespace {

// grid (groups, 1, replicas): header words 0..3 of one level and the group's qualifying roots.  header: the level's
// record of replica r at header + r stride.  Static LDS: 8 + 4 x 4 = 24 bytes.
__global__ void __launch_bounds__(256) k_component_count(long long nsites, const int* __restrict__ parent, const int* __restrict__ size, long long min_size,
                                                         unsigned long long* __restrict__ header, long long stride, unsigned* __restrict__ counts) {
  using namespace component_limits;
  __shared__ unsigned long long sh[3];             // one array: 24 bytes whatever the compiler aligns arrays to
  unsigned* sh_cnt = reinterpret_cast<unsigned*>(sh + 1);   // components, occupied sites, qualifying components
  const int tid = (int)threadIdx.x;
  if (tid == 0) sh[0] = 0ull;
  if (tid < 3) sh_cnt[tid] = 0u;
  __syncthreads();
  const int* __restrict__ par = parent + (long long)blockIdx.z * nsites;
  const int* __restrict__ sz = size + (long long)blockIdx.z * nsites;
  unsigned ncomp = 0u, nocc = 0u, nqual = 0u;      // wave-uniform
  unsigned long long vqual = 0ull;
#pragma unroll
  for (int k = 0; k < kRankSites / 256; ++k) {
    const long long p = (long long)blockIdx.x * kRankSites + k * 256 + tid;
    const int up = p < nsites ? par[p] : -1;
    const bool is_root = up >= 0 && up == (int)p;
    const int s = is_root ? sz[p] : 0;
    const bool qualifies = is_root && (long long)s >= min_size;
    nocc += (unsigned)__popcll(__ballot(up >= 0));
    ncomp += (unsigned)__popcll(__ballot(is_root));
    nqual += (unsigned)__popcll(__ballot(qualifies));
    if (qualifies) vqual += (unsigned long long)s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) vqual += __shfl_down(vqual, off, 64);
  if ((tid & 63) == 0) {
    if (ncomp) atomicAdd(&sh_cnt[0], ncomp);
    if (nocc) atomicAdd(&sh_cnt[1], nocc);
    if (nqual) atomicAdd(&sh_cnt[2], nqual);
    if (vqual) atomicAdd(&sh[0], vqual);
  }
  __syncthreads();
  unsigned long long* out = header + (long long)blockIdx.z * stride;
  if (tid < 3) {
    const unsigned n = sh_cnt[tid];
    if (n) atomicAdd(&out[tid], (unsigned long long)n);
    if (tid == 2) counts[(long long)blockIdx.z * gridDim.x + blockIdx.x] = n;
  } else if (tid == 64) {
    if (sh[0]) atomicAdd(&out[3], sh[0]);
  }
}

// grid (1, 1, replicas): counts[replica][groups] become their exclusive prefix sums.  Static LDS: 16 bytes.
__global__ void __launch_bounds__(256) k_component_scan(unsigned* __restrict__ counts, int groups) {
  __shared__ unsigned sh_wave[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* c = counts + (long long)blockIdx.z * groups;
  unsigned carry = 0u;                             // the same in every thread
  for (int base = 0; base < groups; base += 256) {
    const int i = base + tid;
    const unsigned v = i < groups ? c[i] : 0u;
    unsigned incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) sh_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) before += sh_wave[w]; total += sh_wave[w]; }
    if (i < groups) c[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
}

// grid (groups, 1, replicas), k_component_count's: a qualifying root's rank; label and size into row rank < rows; the
// root's slot into its size word.  rows_out: the level's first row of replica r at rows_out + r stride.  Static LDS: 64 bytes.
__global__ void __launch_bounds__(256) k_component_rank(long long nsites, const int* __restrict__ parent, int* __restrict__ size, long long min_size, int rows,
                                                        unsigned long long* __restrict__ rows_out, long long stride, const unsigned* __restrict__ counts) {
  using namespace component_limits;
  constexpr int kPer = kRankSites / 256;
  __shared__ unsigned sh_wave[4 * kPer];           // [k][wave]: the order of p
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* __restrict__ par = parent + (long long)blockIdx.z * nsites;
  int* __restrict__ sz = size + (long long)blockIdx.z * nsites;
  bool is_root[kPer], qualifies[kPer];
  int s[kPer];
  unsigned before[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const long long p = (long long)blockIdx.x * kRankSites + k * 256 + tid;
    const int up = p < nsites ? par[p] : -1;
    is_root[k] = up >= 0 && up == (int)p;
    s[k] = is_root[k] ? sz[p] : 0;
    qualifies[k] = is_root[k] && (long long)s[k] >= min_size;
    const unsigned long long b = __ballot(qualifies[k]);
    before[k] = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) sh_wave[k * 4 + wave] = (unsigned)__popcll(b);
  }
  __syncthreads();
  const unsigned base = counts[(long long)blockIdx.z * gridDim.x + blockIdx.x];
  unsigned long long* out = rows_out + (long long)blockIdx.z * stride;
  unsigned run = base;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w == wave && is_root[k]) {
        const long long p = (long long)blockIdx.x * kRankSites + k * 256 + tid;
        int slot = -1;
        if (qualifies[k]) {
          const unsigned rank = run + before[k];
          if (rank < (unsigned)rows) {
            slot = (int)rank;
            out[(long long)slot * kRowWords + kLabel] = (unsigned long long)p;
            out[(long long)slot * kRowWords + kSize] = (unsigned long long)s[k];
          }
        }
        sz[p] = slot;
      }
      run += sh_wave[k * 4 + w];
    }
  }
}

// what the two brick kernels share: an in-range occupied site's key and its component's slot (-1: not tabulated)
struct ComponentSite { int key, slot; };
__device__ inline ComponentSite component_site(const ClusterBox& B, int x0, int y0, int z0, int i, int up, const int* __restrict__ par,
                                               const int* __restrict__ sz, int rows) {
  ComponentSite c{-1, -1};
  if (up < 0) return c;
  const int k = component_key(B, x0, y0, z0, up);
  const int slot = sz[par[up]];                    // the global root's word: its slot; a defect's stray value is out of range or harmless
  if (slot < 0 || slot >= rows) return c;
  c.key = k < 0 ? i : k; c.slot = slot;
  return c;
}

// grid (bricks, 1, replicas), 256 threads, two sites per thread.  Static LDS: 512 x (4 + 4 + 4) = 6144 bytes.
__global__ void __launch_bounds__(256) k_component_masks(ClusterBox B, const int* __restrict__ parent, const int* __restrict__ size, int rows,
                                                         unsigned long long* __restrict__ masks) {
  using namespace cluster_limits;
  __shared__ unsigned sh_x[kBrick];                // bit lx
  __shared__ unsigned sh_yz[kBrick];               // bit ly, bit 4 + lz
  __shared__ int sh_slot[kBrick];
  const int tid = (int)threadIdx.x;
  const int nbx = (B.nx + kBx - 1) / kBx, nby = (B.ny + kBy - 1) / kBy;
  const int bi = (int)blockIdx.x;
  const int x0 = (bi % nbx) * kBx, y0 = ((bi / nbx) % nby) * kBy, z0 = (bi / (nbx * nby)) * kBz;
  const long long nsites = (long long)B.nx * B.ny * B.nz;
  const int* __restrict__ par = parent + (long long)blockIdx.z * nsites;
  const int* __restrict__ sz = size + (long long)blockIdx.z * nsites;
#pragma unroll
  for (int k = 0; k < 2; ++k) { const int i = tid + k * kThreads; sh_x[i] = 0u; sh_yz[i] = 0u; sh_slot[i] = -1; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kThreads;
    const int lx = i & (kBx - 1), ly = (i / kBx) & (kBy - 1), lz = i / (kBx * kBy);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x >= B.nx || y >= B.ny || z >= B.nz) continue;
    const ComponentSite c = component_site(B, x0, y0, z0, i, par[((long long)z * B.ny + y) * B.nx + x], par, sz, rows);
    if (c.key < 0) continue;
    atomicOr(&sh_x[c.key], 1u << lx);
    atomicOr(&sh_yz[c.key], (1u << ly) | (16u << lz));
    sh_slot[c.key] = c.slot;                       // every writer of a key writes the same slot
  }
  __syncthreads();
  const int wx = component_mask_words(B.nx), wy = component_mask_words(B.ny);
  const long long slot_words = component_slot_words(B);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kThreads;
    const int slot = sh_slot[i];
    if (slot < 0) continue;
    unsigned long long* m = masks + ((long long)blockIdx.z * rows + slot) * slot_words;
    const unsigned yz = sh_yz[i];
    atomicOr(&m[x0 >> 6], (unsigned long long)sh_x[i] << (x0 & 63));
    atomicOr(&m[wx + (y0 >> 6)], (unsigned long long)(yz & 15u) << (y0 & 63));
    atomicOr(&m[wx + wy + (z0 >> 6)], (unsigned long long)(yz >> 4) << (z0 & 63));
  }
}

// grid (replicas x rows x 3 / 256): origin and extent of one axis of one slot into the row, the mask cleared.
// rows_out: the level's first row of replica r at rows_out + r stride.
__global__ void __launch_bounds__(256) k_component_origin(ClusterBox B, int nrep, int rows, unsigned long long* __restrict__ masks,
                                                          unsigned long long* __restrict__ rows_out, long long stride) {
  using namespace component_limits;
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= nrep * rows * 3) return;
  const int axis = t % 3, slot = (t / 3) % rows, rep = t / (3 * rows);
  const int wx = component_mask_words(B.nx), wy = component_mask_words(B.ny);
  const int n = axis == 0 ? B.nx : (axis == 1 ? B.ny : B.nz);
  unsigned long long* w = masks + ((long long)rep * rows + slot) * component_slot_words(B) + (axis == 0 ? 0 : (axis == 1 ? wx : wx + wy));
  long long origin, extent;
  component_arc(w, n, &origin, &extent);
  for (int i = 0; i < component_mask_words(n); ++i) w[i] = 0ull;
  unsigned long long* row = rows_out + (long long)rep * stride + (long long)slot * kRowWords;
  row[kOrigin + axis] = (unsigned long long)origin;
  row[kExtent + axis] = (unsigned long long)extent;
}

// grid (bricks, 1, replicas), 256 threads, two sites per thread.  Static LDS: 512 x (10 x 8 + 4) = 43008 bytes.
__global__ void __launch_bounds__(256) k_component_moments(ClusterBox B, const int* __restrict__ parent, const int* __restrict__ size, int rows,
                                                           unsigned long long* __restrict__ rows_out, long long stride) {
  using namespace cluster_limits;
  using namespace component_limits;
  __shared__ unsigned long long sh_sum[kSums][kBrick];
  __shared__ int sh_slot[kBrick];
  const int tid = (int)threadIdx.x;
  const int nbx = (B.nx + kBx - 1) / kBx, nby = (B.ny + kBy - 1) / kBy;
  const int bi = (int)blockIdx.x;
  const int x0 = (bi % nbx) * kBx, y0 = ((bi / nbx) % nby) * kBy, z0 = (bi / (nbx * nby)) * kBz;
  const long long nsites = (long long)B.nx * B.ny * B.nz;
  const int* __restrict__ par = parent + (long long)blockIdx.z * nsites;
  const int* __restrict__ sz = size + (long long)blockIdx.z * nsites;
  unsigned long long* out = rows_out + (long long)blockIdx.z * stride;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kThreads;
#pragma unroll
    for (int j = 0; j < kSums; ++j) sh_sum[j][i] = 0ull;
    sh_slot[i] = -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {                    // no thread leaves this loop early: the wave votes below
    const int i = tid + k * kThreads;
    const int lx = i & (kBx - 1), ly = (i / kBx) & (kBy - 1), lz = i / (kBx * kBy);
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    ComponentSite c{-1, -1};
    if (x < B.nx && y < B.ny && z < B.nz) c = component_site(B, x0, y0, z0, i, par[((long long)z * B.ny + y) * B.nx + x], par, sz, rows);
    unsigned long long v[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) v[j] = 0ull;
    if (c.key >= 0) {
      const unsigned long long* row = out + (long long)c.slot * kRowWords;
      const unsigned long long dx = (unsigned long long)component_offset(x, (int)row[kOrigin], B.nx);
      const unsigned long long dy = (unsigned long long)component_offset(y, (int)row[kOrigin + 1], B.ny);
      const unsigned long long dz = (unsigned long long)component_offset(z, (int)row[kOrigin + 2], B.nz);
      unsigned long long faces = 0ull;
#pragma unroll
      for (int d = -1; d <= 1; d += 2) {
        faces += par[((long long)z * B.ny + y) * B.nx + component_wrap(x, d, B.nx)] < 0;
        faces += par[((long long)z * B.ny + component_wrap(y, d, B.ny)) * B.nx + x] < 0;
        faces += par[((long long)component_wrap(z, d, B.nz) * B.ny + y) * B.nx + x] < 0;
      }
      v[0] = dx; v[1] = dy; v[2] = dz; v[3] = dx * dx; v[4] = dy * dy; v[5] = dz * dz; v[6] = dx * dy; v[7] = dx * dz; v[8] = dy * dz; v[9] = faces;
      sh_slot[c.key] = c.slot;                     // every writer of a key writes the same slot
    }
    const unsigned long long active = __ballot(c.key >= 0);
    if (active == 0ull) continue;                  // wave-uniform
    const int key0 = __shfl(c.key, __ffsll((long long)active) - 1, 64);
    if (__all(c.key < 0 || c.key == key0)) {       // one key in the wave: one LDS add per word
#pragma unroll
      for (int j = 0; j < kSums; ++j) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_down(v[j], off, 64);
        if ((tid & 63) == 0 && v[j]) atomicAdd(&sh_sum[j][key0], v[j]);
      }
    } else if (c.key >= 0) {
#pragma unroll
      for (int j = 0; j < kSums; ++j)
        if (v[j]) atomicAdd(&sh_sum[j][c.key], v[j]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kThreads;
    const int slot = sh_slot[i];
    if (slot < 0) continue;
    unsigned long long* row = out + (long long)slot * kRowWords;
#pragma unroll
    for (int j = 0; j < kSums; ++j) {
      const unsigned long long s = sh_sum[j][i];
      if (s) atomicAdd(&row[kSum + j], s);
    }
  }
}

// one thread per (replica, level, header or row): the staging into the slot and back to zero.  n: replicas x levels.
__global__ void __launch_bounds__(256) k_component_finish(unsigned long long* __restrict__ totals, long long* __restrict__ out, int n, int rows) {
  using namespace component_limits;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * (rows + 1)) return;
  const long long rec = t / (rows + 1);
  const int item = (int)(t % (rows + 1));
  const long long at = rec * component_words(rows) + (item ? kHeader + (long long)(item - 1) * kRowWords : 0);
  unsigned long long* s = totals + at;
  long long* o = out + at;
  if (item == 0) {
    const long long nqual = (long long)s[2];
    for (int w = 0; w < kHeader; ++w) { o[w] = (long long)s[w]; s[w] = 0ull; }
    o[4] = nqual < rows ? nqual : rows;
  } else {
    const bool used = s[kSize] != 0ull;             // a tabulated component has a size >= min_size >= 1
    for (int w = 0; w < kRowWords; ++w) { o[w] = used ? (long long)s[w] : 0; s[w] = 0ull; }
    if (!used) o[kLabel] = -1;
  }
}

int component_create(bflbm_ctx* c, bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int connectivity, long long min_size,
                     int rows, int every, long long capacity, bflbm_component** out) {
  const char* call = b ? "bflbm_batch_component_create" : "bflbm_component_create";
  if (component_refuse_args(call, source, var, nlevels, levels, side, connectivity, min_size, rows)) return 1;
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_component_create", "component trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if (component_refuse_sites(call, G.nx, G.ny, G.nz)) return 1;

  std::unique_ptr<bflbm_component> t(new bflbm_component());
  recorder_bind(t.get(), c, b, every);
  t->B = ClusterBox{G.nx, G.ny, G.nz, connectivity};
  t->nsites = (long long)G.nx * G.ny * G.nz;
  t->min_size = min_size; t->rows = rows;
  t->fs = field_select(b != nullptr, source, 1, &var);
  t->L = morph_levels(nlevels, levels, side);

  const size_t per = t->words();
  const std::string shape = " x " + std::to_string(nlevels) + " levels x (6 + " + std::to_string(rows) + " rows x 18) words";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the arrays
  const size_t sb = per * sizeof(long long);
  const size_t ab = (size_t)t->nrep * (size_t)t->nsites * sizeof(int);
  const size_t fb = b ? (size_t)t->nrep * (size_t)t->nsites * sizeof(double) : 0;
  const size_t mb = t->mask_words() * sizeof(unsigned long long);
  const size_t cb = (size_t)t->nrep * (size_t)component_groups(t->nsites) * sizeof(unsigned);
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->parent, ab);
  if (e == hipSuccess) e = hipMalloc((void**)&t->size, ab);
  if (e == hipSuccess) e = hipMalloc((void**)&t->masks, mb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->counts, cb);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (field %zu bytes, parents %zu, slots %zu, masks %zu, counts %zu; then records %zu x %lld + staging %zu): %s", call,
                fb, ab, ab, mb, cb, sb, capacity, sb, hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, per, shape.c_str())) return 1;
  // the staging is the store's stage buffer: zeroed, like the masks, after the owner's list took the trace, as the cluster trace does
  bflbm_component* m = t.release();
  e = hipMemsetAsync(m->d_stage, 0, sb, recorder_stream(m));
  if (e == hipSuccess) e = hipMemsetAsync(m->masks, 0, mb, recorder_stream(m));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(m);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = m;
  return 0;
}

}  // namespace

// enqueue the observation, the nine launches per level and the finishing launch of the resident state into slot n
int bflbm_component::record() {
  using namespace component_limits;
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "component trace sample", &dense, &rep_stride)) return 1;
  const double* vol = dense + (long long)fs.vol.vol[0] * nsites;
  const ClusterArrays A = arrays();
  const int groups = (int)component_groups(nsites);
  const dim3 per_group((unsigned)groups, 1, (unsigned)nrep), per_brick((unsigned)cluster_bricks(B.nx, B.ny, B.nz), 1, (unsigned)nrep);
  const dim3 per_axis((unsigned)((nrep * rows * 3 + 255) / 256));
  const long long W = component_words(rows), stride = (long long)L.n * W;
  for (int l = 0; l < L.n; ++l) {
    unsigned long long* level = totals() + (long long)l * W;
    unsigned long long* first_row = level + kHeader;
    if (cluster_label_level(A, vol, rep_stride, L.t[l], L.side, level + kCapped, stride)) return 1;
    if (cluster_resolve_level(A, level + kCapped, stride)) return 1;
    hipLaunchKernelGGL(k_component_count, per_group, dim3(256), 0, stream, nsites, (const int*)parent, (const int*)size, min_size, level, stride, counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_component_scan, dim3(1, 1, (unsigned)nrep), dim3(256), 0, stream, counts, groups);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_component_rank, per_group, dim3(256), 0, stream, nsites, (const int*)parent, size, min_size, rows, first_row, stride,
                       (const unsigned*)counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_component_masks, per_brick, dim3(256), 0, stream, B, (const int*)parent, (const int*)size, rows, masks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_component_origin, per_axis, dim3(256), 0, stream, B, nrep, rows, masks, first_row, stride);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_component_moments, per_brick, dim3(256), 0, stream, B, (const int*)parent, (const int*)size, rows, first_row, stride);
    HIP_TRY(hipGetLastError());
  }
  const int n = nrep * L.n;
  hipLaunchKernelGGL(k_component_finish, dim3((unsigned)(((long long)n * (rows + 1) + 255) / 256)), dim3(256), 0, stream, totals(),
                     reinterpret_cast<long long*>(store_slot(this)), n, rows);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_component_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels, int side, int connectivity, long long min_size, int rows,
                           int every, long long capacity, bflbm_component** out) {
  if (!c || !levels || !out) return fail("bflbm_component_create: null argument");
  return component_create(c, nullptr, source, var, nlevels, levels, side, connectivity, min_size, rows, every, capacity, out);
}
int bflbm_batch_component_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int connectivity, long long min_size,
                                 int rows, int every, long long capacity, bflbm_component** out) {
  if (!b || !levels || !out) return fail("bflbm_batch_component_create: null argument");
  return component_create(nullptr, b, source, var, nlevels, levels, side, connectivity, min_size, rows, every, capacity, out);
}

int bflbm_component_destroy(bflbm_component* t) { return store_destroy(t); }
int bflbm_component_sample(bflbm_component* t) { return store_sample(t, "bflbm_component"); }
int bflbm_component_reset(bflbm_component* t) { return store_reset(t, "bflbm_component"); }
int bflbm_component_count(const bflbm_component* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_component", nsamples, nreplicas); }
int bflbm_component_read(bflbm_component* t, long long first, long long count, long long* record, long long* steps) {
  return store_read(t, "bflbm_component", first, count, reinterpret_cast<double*>(record), steps);   // 8-byte slots, copied bit for bit
}

int bflbm_component_geometry(const bflbm_component* t, int* nlevels, int* connectivity, long long* min_size, int* rows, int* header_words, int* row_words,
                             int* launches) {
  if (!t) return fail("bflbm_component_geometry: null argument");
  if (nlevels) *nlevels = t->L.n;
  if (connectivity) *connectivity = t->B.conn;
  if (min_size) *min_size = t->min_size;
  if (rows) *rows = t->rows;
  if (header_words) *header_words = component_limits::kHeader;
  if (row_words) *row_words = component_limits::kRowWords;
  if (launches) *launches = component_limits::kLaunches;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_COMPONENTS_HOST_ONLY

#endif  // BFLBM_COMPONENTS_H_
