// bflbm_cluster.h -- cluster traces: the connected components of the set {v >= level} or {v < level} of one observed hydrovs
// or hydrovsbar variable at 1 to 8 levels, under 6- or 26-connectivity on the periodic box, recorded on the device as a
// time series of 38 64-bit integers per level for a lone single-slab context or every replica of a batch
// (include/bflbm.h, "Cluster traces": the definition and the layout of a sample are stated there and only there).  How
// many domains there are and how large each one is are questions the morphology trace answers only through chi; without
// this a user downloads the field per sample and labels on the host.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   of the one variable, exactly as the morphology trace takes it (fields_observe),
//   per level, one after another through the same two arrays parent and size, int32 [replica][nsites]:
//   k_cluster_local                 grid (bricks, 1, replicas), 256 threads, one workgroup per brick of 32 x 4 x 4 sites
//                                   (two sites per thread).  It loads the occupancy, unites in LDS, with LDS atomics, the
//                                   links that lie inside the brick and do not wrap, and writes per site the global index
//                                   of its brick-local root into parent (-1: unoccupied) and per site the size of the
//                                   local component where the site is its root, else 0.  The brick-local index
//                                   (lz 4 + ly) 32 + lx is monotone in p, so the smallest stays the smallest.
//   k_cluster_merge                 one thread per site: every forward link that crosses a brick face or wraps (those of a
//                                   brick with itself included), united in global memory.
//   k_cluster_resolve               one thread per site: a brick-local root finds its global root, adds its local size to
//                                   the global root's and points at it.  The adds per component are the bricks it
//                                   touches, not its sites.
//   k_cluster_stats                 1024 sites per workgroup: over the global roots (parent[p] == p) the words 0, 1, 4 and
//                                   the histogram bin summed per wave and workgroup, one 64-bit global add per non-zero
//                                   counter and workgroup; words 2 and 3 as one packed 64-bit maximum,
//                                   (size << 32) | (0xffffffff - label).
//   and once, k_cluster_finish      the totals of all levels into the slot, the packed maximum unpacked, the totals cleared.
// The phases are separated by launches, not by a grid barrier: a stuck barrier is a hang.
// find and union are plain inline functions over a memory policy (load, min_old, capped); the kernels instantiate them with
// LDS and global atomics, tests/cluster_main.cpp with sequential stand-ins and runs them under sanitizers.
// Invariant: parent[p] <= p throughout, so a root is the smallest index of its tree, and at the end, every link united,
// of its component.
// Coherence (MI355X: a CU's L1 is never refreshed by another CU's stores, the L2s of different XCDs are not coherent for
// plain accesses within a kernel): inside k_cluster_merge and k_cluster_resolve every access to parent is a relaxed
// agent-scope atomic, a load that bypasses L1 or a read-modify-write performed at the point of coherence.  Nothing
// depends on a load being fresh: (1) parents only decrease (every write is an atomic minimum with a smaller index);
// (2) a stale parent is an older ancestor of the same tree, or, between the minimum that re-pointed a non-root and the
// union that repairs it, a site the same thread is about to unite with that tree; either way following it only ever
// reaches sites that the finished kernel has in one tree; (3) every link is decided by the value the atomic minimum
// returns: `old == a` says that this call made the root a a child, anything else that a had been linked meanwhile and
// the union goes on with (old, b).  What a later launch reads is ordered by the launch boundary, so the local, stats,
// finish and flatten kernels use plain accesses for what earlier launches wrote.
// Termination: find follows strictly decreasing indices and so loads at most p + 1 <= nsites times.  In union the larger
// of the two sites is replaced by a strictly smaller one (old < a, and find never increases), so the maximum of the pair
// falls every turn: at most nsites turns.  Both loops also carry that bound as a hard cap; reaching it adds one to word 5
// of the sample and leaves the loop, so a defect is a failed assertion, never a hang.
// Memory: parent and size, 8 bytes per site and replica; a batch also the dense field, as the morphology trace.
// Expected traffic per site and level, derived: local 8 (field) + 8 (parent, size) bytes; merge 4 plus the neighbours'
// parents of the 45 % (26) or 40 % (6) of sites on a forward brick face, through the caches; resolve 4 (size) and the
// chains of the roots only; stats 8: about 32 bytes against the 608 of a step.  The brick is an untimed heuristic.
// Out of scope: rings (a link crosses the slab boundary: no bflbm_ring_cluster_create), per-component sums of a second
// variable, wrapping (winding) detection, tracking between samples on the device, 18-connectivity, a noise source.  Per
// component size, origin, extent (spanning), integer moments and area are the component trace's (bflbm_components.h), which
// calls cluster_label_level and cluster_resolve_level below.
// Host part: plain C++17 on top of bflbm_morph.h's host part (the levels, the refusals).  A stand-alone program defines
// BFLBM_CLUSTER_HOST_ONLY (and the MORPH and FIELDSEL ones) and includes it after bflbm_morph.h.  HIP part: the lifecycle
// and the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by bflbm.hip after
// bflbm_morph.h.
#ifndef BFLBM_CLUSTER_H_
#define BFLBM_CLUSTER_H_

#include <algorithm>
#include <cmath>

#ifdef BFLBM_CLUSTER_HOST_ONLY
#define BFLBM_CLUSTER_FN inline
#else
#define BFLBM_CLUSTER_FN __host__ __device__ inline
#endif

namespace cluster_limits {
constexpr int kWords = 38;                       // 64-bit words of a level's record
constexpr int kBins = 32, kFirstBin = 6;         // components with 2^b <= s < 2^(b+1) at word 6 + b
constexpr int kCapped = 5;                       // the word that counts loops that hit their cap
constexpr int kBx = 32, kBy = 4, kBz = 4;        // the brick
constexpr int kBrick = kBx * kBy * kBz;
constexpr int kThreads = 256;
constexpr int kStatsSites = 4 * kThreads;        // sites of a workgroup of k_cluster_stats
constexpr int kLaunches = 4;                     // per level: local, merge, resolve, stats
constexpr long long kMaxSites = 2147483647LL;    // labels are 32-bit
static_assert(kBrick == 2 * kThreads, "two sites per thread");
static_assert(kFirstBin + kBins == kWords, "the histogram ends the record");
}

// the box and the connectivity; a by-value kernel parameter
struct ClusterBox { int nx, ny, nz, conn; };

BFLBM_CLUSTER_FN int cluster_ndirs(int conn) { return conn == 6 ? 3 : 13; }

// One step of a coordinate: q is the periodic neighbour of c (an extent of 1 is its own neighbour); true where the step
// neither wraps nor leaves the brick of extent b.
BFLBM_CLUSTER_FN bool cluster_step(int c, int d, int n, int b, int* q) {
  int t = c + d;
  const bool inside = t >= 0 && t < n && t / b == c / b;
  if (t < 0) t += n; else if (t >= n) t -= n;
  *q = t;
  return inside;
}

// The linear index of the neighbour of (x, y, z) along the forward direction k of the connectivity: the 3 or 13
// directions (dx, dy, dz) with (dz, dy, dx) lexicographically positive.  *local: the link lies inside one brick and does
// not wrap (k_cluster_local's); else it is k_cluster_merge's.
BFLBM_CLUSTER_FN int cluster_neighbour(const ClusterBox& B, int x, int y, int z, int k, bool* local) {
  using namespace cluster_limits;
  const int j = B.conn == 6 ? (k == 0 ? 14 : (k == 1 ? 16 : 22)) : 14 + k;      // (dz + 1) 9 + (dy + 1) 3 + dx + 1
  int xq, yq, zq;
  const bool ix = cluster_step(x, j % 3 - 1, B.nx, kBx, &xq);
  const bool iy = cluster_step(y, (j / 3) % 3 - 1, B.ny, kBy, &yq);
  const bool iz = cluster_step(z, j / 9 - 1, B.nz, kBz, &zq);
  *local = ix && iy && iz;
  return (zq * B.ny + yq) * B.nx + xq;
}

// The root of p: indices fall strictly along the way, so at most p + 1 <= cap loads.  A policy Mem has int load(int),
// int min_old(int at, int value) (the minimum stored, the value before returned) and void capped().
template <class Mem> BFLBM_CLUSTER_FN int cluster_find(Mem& m, int p, long long cap) {
  for (long long it = 0; it < cap; ++it) {
    const int q = m.load(p);
    if (q == p) return p;
    p = q;
  }
  m.capped();
  return p;
}

// Unite the trees of a and b, lock-free: the larger root becomes a child of the smaller by an atomic minimum.  Where the
// larger site had meanwhile been linked (old != a), its parent is now min(old, b) and the link that may have been cut,
// a -- old, is restored by going on with (old, b).  The larger of the pair falls every turn: at most cap turns.
template <class Mem> BFLBM_CLUSTER_FN void cluster_union(Mem& m, int a, int b, long long cap) {
  for (long long it = 0; it < cap; ++it) {
    a = cluster_find(m, a, cap);
    b = cluster_find(m, b, cap);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = m.min_old(a, b);
    if (old == a) return;
    a = old;
  }
  m.capped();
}

// the histogram bin of a size s >= 1, and the packed maximum: the larger size wins, among equals the smaller label
BFLBM_CLUSTER_FN int cluster_bin(int s) { int b = 0; while (s >>= 1) ++b; return b; }
BFLBM_CLUSTER_FN unsigned long long cluster_pack(int size, int label) { return ((unsigned long long)size << 32) | (0xffffffffull - (unsigned)label); }
BFLBM_CLUSTER_FN long long cluster_packed_size(unsigned long long k) { return (long long)(k >> 32); }
BFLBM_CLUSTER_FN long long cluster_packed_label(unsigned long long k) { return k ? (long long)(0xffffffffull - (k & 0xffffffffull)) : -1; }

namespace {

// What every creation call refuses about its arguments: the morphology trace's refusals in its order, then the connectivity.
int cluster_refuse_args(const char* call, int source, int var, int nlevels, const double* levels, int side, int connectivity) {
  if (morph_refuse_args(call, source, var, nlevels, levels, side)) return 1;
  if (connectivity != 6 && connectivity != 26) return fail("%s: connectivity must be 6 or 26 (got %d)", call, connectivity);
  return 0;
}
int cluster_refuse_sites(const char* call, int nx, int ny, int nz) {
  const long long n = (long long)nx * ny * nz;
  if (n > cluster_limits::kMaxSites) return fail("%s: %lld sites exceed %lld (labels are 32-bit)", call, n, cluster_limits::kMaxSites);
  return 0;
}

inline long long cluster_bricks(int nx, int ny, int nz) {
  using namespace cluster_limits;
  return (long long)((nx + kBx - 1) / kBx) * ((ny + kBy - 1) / kBy) * ((nz + kBz - 1) / kBz);
}

}  // namespace

#ifndef BFLBM_CLUSTER_HOST_ONLY

#include <memory>
#include <string>

// What the launches of one level work on: a stream, the replicas' box and the two arrays.  The cluster trace and the
// component trace (bflbm_components.h) both label through cluster_label_level and cluster_resolve_level.
struct ClusterArrays { hipStream_t stream; int nrep; long long nsites; ClusterBox B; int* parent; int* size; };

struct bflbm_cluster : bflbm_sample_store {  // d_rec [capacity][nrep][nlevels][38] as long long, d_stage: the totals and one word more
  ClusterBox B;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar; one variable
  MorphLevels L;
  double* fields = nullptr;         // a batch: [nrep][nsites]
  int* parent = nullptr;            // [nrep][nsites]
  int* size = nullptr;              // [nrep][nsites]; bflbm_cluster_labels flattens into it
  bflbm_cluster() : bflbm_sample_store("cluster trace", "bflbm_cluster") {}
  ~bflbm_cluster() override {
    if (!fields && !parent && !size) return;
    hipSetDevice(device);
    if (fields) hipFree(fields);
    if (parent) hipFree(parent);
    if (size) hipFree(size);
  }
  unsigned long long* totals() const { return reinterpret_cast<unsigned long long*>(d_stage); }
  size_t words() const { return (size_t)nrep * L.n * cluster_limits::kWords; }   // the totals; the word after them: the caps of a labels call
  ClusterArrays arrays() const { return ClusterArrays{recorder_stream(this), nrep, nsites, B, parent, size}; }
  int observe(const double** vol, long long* rep_stride);
  int label_level(const double* vol, long long rep_stride, int l, unsigned long long* capped, long long capped_stride);
  int record() override;
};

namespace {

// the policies of find and union: the brick's parents in LDS, a replica's in global memory
struct ClusterLdsMem {
  int* parent;
  unsigned long long* caps;
  __device__ int load(int p) const { return __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ int min_old(int p, int v) const { return __hip_atomic_fetch_min(parent + p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ void capped() const { atomicAdd(caps, 1ull); }
};
struct ClusterGlobalMem {
  int* parent;
  unsigned long long* caps;
  __device__ int load(int p) const { return __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ int min_old(int p, int v) const { return __hip_atomic_fetch_min(parent + p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ void capped() const { atomicAdd(caps, 1ull); }
};

// grid (bricks, 1, replicas), 256 threads.  field: the dense volume [nz][ny][nx] of replica r at field + r rep_stride.
__global__ void __launch_bounds__(256) k_cluster_local(const double* __restrict__ field, long long rep_stride, ClusterBox B, double level, int side,
                                                       int* __restrict__ parent, int* __restrict__ size, unsigned long long* caps, long long caps_stride) {
  using namespace cluster_limits;
  __shared__ int sh_parent[kBrick];
  __shared__ int sh_count[kBrick];
  const int tid = (int)threadIdx.x;
  const int nbx = (B.nx + kBx - 1) / kBx, nby = (B.ny + kBy - 1) / kBy;
  const int bi = (int)blockIdx.x;
  const int x0 = (bi % nbx) * kBx, y0 = ((bi / nbx) % nby) * kBy, z0 = (bi / (nbx * nby)) * kBz;
  const long long nsites = (long long)B.nx * B.ny * B.nz;
  const long long rep = (long long)blockIdx.z * nsites;
  const double* __restrict__ vol = field + (long long)blockIdx.z * rep_stride;
  ClusterLdsMem m{sh_parent, caps + (long long)blockIdx.z * caps_stride};

  int xs[2], ys[2], zs[2];
  bool in[2], occ[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kThreads;
    xs[k] = x0 + (i & (kBx - 1)); ys[k] = y0 + ((i / kBx) & (kBy - 1)); zs[k] = z0 + i / (kBx * kBy);
    in[k] = xs[k] < B.nx && ys[k] < B.ny && zs[k] < B.nz;
    occ[k] = false;
    if (in[k]) {
      const double v = vol[((long long)zs[k] * B.ny + ys[k]) * B.nx + xs[k]];
      occ[k] = side ? v < level : v >= level;          // a NaN fails both
    }
    sh_parent[i] = occ[k] ? i : -1;
    sh_count[i] = 0;
  }
  __syncthreads();
  const int ndirs = cluster_ndirs(B.conn);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!occ[k]) continue;
    const int i = tid + k * kThreads;
    for (int d = 0; d < ndirs; ++d) {
      bool local;
      const int q = cluster_neighbour(B, xs[k], ys[k], zs[k], d, &local);
      if (!local) continue;
      // the neighbour's brick-local index: same brick, so its offsets from (x0, y0, z0) are in range
      const int zq = q / (B.nx * B.ny), yq = (q - zq * B.nx * B.ny) / B.nx, xq = q - (zq * B.ny + yq) * B.nx;
      const int j = ((zq - z0) * kBy + (yq - y0)) * kBx + (xq - x0);
      if (m.load(j) >= 0) cluster_union(m, i, j, kBrick);
    }
  }
  __syncthreads();
  int root[2] = {-1, -1};
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (occ[k]) { root[k] = cluster_find(m, tid + k * kThreads, kBrick); atomicAdd(&sh_count[root[k]], 1); }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (!in[k]) continue;
    const int i = tid + k * kThreads;
    const long long p = ((long long)zs[k] * B.ny + ys[k]) * B.nx + xs[k];
    const int r = root[k];
    const int gr = r < 0 ? -1 : ((z0 + r / (kBx * kBy)) * B.ny + y0 + ((r / kBx) & (kBy - 1))) * B.nx + x0 + (r & (kBx - 1));
    parent[rep + p] = gr;
    size[rep + p] = r == i ? sh_count[i] : 0;
  }
}

// grid (sites / 256, 1, replicas): the forward links that cross a brick face or wrap
__global__ void __launch_bounds__(256) k_cluster_merge(ClusterBox B, int* parent, unsigned long long* caps, long long caps_stride) {
  const long long nsites = (long long)B.nx * B.ny * B.nz;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nsites) return;
  const int p = (int)t;
  ClusterGlobalMem m{parent + (long long)blockIdx.z * nsites, caps + (long long)blockIdx.z * caps_stride};
  const int up = m.load(p);
  if (up < 0) return;
  const int z = p / (B.nx * B.ny), y = (p - z * B.nx * B.ny) / B.nx, x = p - (z * B.ny + y) * B.nx;
  const int ndirs = cluster_ndirs(B.conn);
  for (int d = 0; d < ndirs; ++d) {
    bool local;
    const int q = cluster_neighbour(B, x, y, z, d, &local);
    if (local || q == p) continue;
    const int uq = m.load(q);
    if (uq >= 0) cluster_union(m, up, uq, nsites);
  }
}

// grid (sites / 256, 1, replicas): a brick-local root adds its size to its global root's and points at it
__global__ void __launch_bounds__(256) k_cluster_resolve(long long nsites, int* parent, int* size, unsigned long long* caps, long long caps_stride) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nsites) return;
  const int p = (int)t;
  int* sz = size + (long long)blockIdx.z * nsites;
  const int s = sz[p];               // the local launch wrote it; only a global root's word is added to here, and a global root reads no further
  if (s <= 0) return;
  ClusterGlobalMem m{parent + (long long)blockIdx.z * nsites, caps + (long long)blockIdx.z * caps_stride};
  const int r = cluster_find(m, p, nsites);
  if (r == p) return;
  atomicAdd(&sz[r], s);
  m.min_old(p, r);
}

// grid (sites / 1024, 1, replicas): the record of one level from the global roots.  totals: the level's 38 words of
// replica r at totals + r totals_stride.  Static LDS: 2 x 8 + 34 x 4 = 152 bytes.
__global__ void __launch_bounds__(256) k_cluster_stats(long long nsites, const int* __restrict__ parent, const int* __restrict__ size,
                                                       unsigned long long* __restrict__ totals, long long totals_stride) {
  using namespace cluster_limits;
  __shared__ unsigned long long sh[2 + (2 + kBins) / 2];   // one array: 152 bytes whatever the compiler aligns arrays to
  unsigned long long* sh_wide = sh;                // sum of s^2, the packed maximum
  unsigned* sh_cnt = reinterpret_cast<unsigned*>(sh + 2);   // components, occupied sites, the bins
  const int tid = (int)threadIdx.x;
  if (tid < 2) sh_wide[tid] = 0ull;
  if (tid < 2 + kBins) sh_cnt[tid] = 0u;
  __syncthreads();
  const int* __restrict__ par = parent + (long long)blockIdx.z * nsites;
  const int* __restrict__ sz = size + (long long)blockIdx.z * nsites;
  unsigned ncomp = 0u, nocc = 0u;                  // wave-uniform
  unsigned long long s2 = 0ull, best = 0ull;
#pragma unroll
  for (int k = 0; k < kStatsSites / kThreads; ++k) {
    const long long p = (long long)blockIdx.x * kStatsSites + k * kThreads + tid;
    const int up = p < nsites ? par[p] : -1;
    const bool is_root = up >= 0 && up == (int)p;
    nocc += (unsigned)__popcll(__ballot(up >= 0));
    ncomp += (unsigned)__popcll(__ballot(is_root));
    if (is_root) {
      const int s = sz[p];
      s2 += (unsigned long long)s * (unsigned long long)s;
      best = max(best, cluster_pack(s, (int)p));
      atomicAdd(&sh_cnt[2 + cluster_bin(s)], 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s2 += __shfl_down(s2, off, 64);
    best = max(best, (unsigned long long)__shfl_down(best, off, 64));
  }
  if ((tid & 63) == 0) {
    if (ncomp) atomicAdd(&sh_cnt[0], ncomp);
    if (nocc) atomicAdd(&sh_cnt[1], nocc);
    if (s2) atomicAdd(&sh_wide[0], s2);
    if (best) atomicMax(&sh_wide[1], best);
  }
  __syncthreads();
  unsigned long long* out = totals + (long long)blockIdx.z * totals_stride;
  if (tid < 2 + kBins) {
    const unsigned n = sh_cnt[tid];
    if (n) atomicAdd(&out[tid < 2 ? tid : kFirstBin + tid - 2], (unsigned long long)n);
  } else if (tid == 64) {
    if (sh_wide[0]) atomicAdd(&out[4], sh_wide[0]);
  } else if (tid == 65) {
    if (sh_wide[1]) atomicMax(&out[2], sh_wide[1]);
  }
}

// one thread per (replica, level): the totals into the slot, the packed maximum unpacked, the totals back to zero
__global__ void __launch_bounds__(256) k_cluster_finish(unsigned long long* __restrict__ totals, long long* __restrict__ out, int n) {
  using namespace cluster_limits;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  unsigned long long* t = totals + (long long)i * kWords;
  long long* o = out + (long long)i * kWords;
  const unsigned long long packed = t[2];
  for (int w = 0; w < kWords; ++w) { o[w] = (long long)t[w]; t[w] = 0ull; }
  o[2] = cluster_packed_size(packed);
  o[3] = cluster_packed_label(packed);
}

// grid (sites / 256, 1, replicas): every site's root into out, -1 where unoccupied; reads the parents only
__global__ void __launch_bounds__(256) k_cluster_flatten(long long nsites, int* parent, int* __restrict__ out, unsigned long long* caps, long long caps_stride) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nsites) return;
  ClusterGlobalMem m{parent + (long long)blockIdx.z * nsites, caps + (long long)blockIdx.z * caps_stride};
  const int up = m.load((int)t);
  out[(long long)blockIdx.z * nsites + t] = up < 0 ? -1 : cluster_find(m, up, nsites);
}

int cluster_create(bflbm_ctx* c, bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int connectivity, int every,
                   long long capacity, bflbm_cluster** out) {
  const char* call = b ? "bflbm_batch_cluster_create" : "bflbm_cluster_create";
  if (cluster_refuse_args(call, source, var, nlevels, levels, side, connectivity)) return 1;
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_cluster_create", "cluster trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if (cluster_refuse_sites(call, G.nx, G.ny, G.nz)) return 1;

  std::unique_ptr<bflbm_cluster> t(new bflbm_cluster());
  recorder_bind(t.get(), c, b, every);
  t->B = ClusterBox{G.nx, G.ny, G.nz, connectivity};
  t->nsites = (long long)G.nx * G.ny * G.nz;
  t->fs = field_select(b != nullptr, source, 1, &var);
  t->L = morph_levels(nlevels, levels, side);

  const size_t per = t->words();
  const std::string shape = " x " + std::to_string(nlevels) + " levels x 38 words";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the arrays
  const size_t sb = per * sizeof(long long);
  const size_t ab = (size_t)t->nrep * (size_t)t->nsites * sizeof(int);
  const size_t fb = b ? (size_t)t->nrep * (size_t)t->nsites * sizeof(double) : 0;
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->parent, ab);
  if (e == hipSuccess) e = hipMalloc((void**)&t->size, ab);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (field %zu bytes, parents %zu, sizes %zu; then records %zu x %lld + totals %zu): %s", call, fb, ab, ab, sb,
                capacity, sb + sizeof(long long), hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, per + 1, shape.c_str())) return 1;
  // the totals are the store's stage buffer: zeroed after the owner's list took the trace, as the morphology trace does
  bflbm_cluster* m = t.release();
  e = hipMemsetAsync(m->d_stage, 0, sb + sizeof(long long), recorder_stream(m));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(m);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = m;
  return 0;
}

// the launches that leave the parents of one level united; `capped`: where replica r's loops count their caps, at capped + r capped_stride
int cluster_label_level(const ClusterArrays& A, const double* vol, long long rep_stride, double level, int side, unsigned long long* capped,
                        long long capped_stride) {
  const dim3 per_site((unsigned)((A.nsites + 255) / 256), 1, (unsigned)A.nrep);
  hipLaunchKernelGGL(k_cluster_local, dim3((unsigned)cluster_bricks(A.B.nx, A.B.ny, A.B.nz), 1, (unsigned)A.nrep), dim3(256), 0, A.stream, vol, rep_stride,
                     A.B, level, side, A.parent, A.size, capped, capped_stride);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_cluster_merge, per_site, dim3(256), 0, A.stream, A.B, A.parent, capped, capped_stride);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the launch after which a global root holds its component's size and every brick-local root points at its global root
int cluster_resolve_level(const ClusterArrays& A, unsigned long long* capped, long long capped_stride) {
  const dim3 per_site((unsigned)((A.nsites + 255) / 256), 1, (unsigned)A.nrep);
  hipLaunchKernelGGL(k_cluster_resolve, per_site, dim3(256), 0, A.stream, A.nsites, A.parent, A.size, capped, capped_stride);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

int bflbm_cluster::observe(const double** vol, long long* rep_stride) {
  const double* dense;
  if (fields_observe(this, fs, fields, "cluster trace sample", &dense, rep_stride)) return 1;
  *vol = dense + (long long)fs.vol.vol[0] * nsites;
  return 0;
}

// level l of this trace through cluster_label_level
int bflbm_cluster::label_level(const double* vol, long long rep_stride, int l, unsigned long long* capped, long long capped_stride) {
  return cluster_label_level(arrays(), vol, rep_stride, L.t[l], L.side, capped, capped_stride);
}

// enqueue the observation, the four launches per level and the finishing launch of the resident state into slot n
int bflbm_cluster::record() {
  using namespace cluster_limits;
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* vol;
  long long rep_stride;
  if (observe(&vol, &rep_stride)) return 1;
  const dim3 per_stats((unsigned)((nsites + kStatsSites - 1) / kStatsSites), 1, (unsigned)nrep);
  const long long stride = (long long)L.n * kWords;
  for (int l = 0; l < L.n; ++l) {
    unsigned long long* level = totals() + (long long)l * kWords;
    if (label_level(vol, rep_stride, l, level + kCapped, stride)) return 1;
    if (cluster_resolve_level(arrays(), level + kCapped, stride)) return 1;
    hipLaunchKernelGGL(k_cluster_stats, per_stats, dim3(256), 0, stream, nsites, (const int*)parent, (const int*)size, level, stride);
    HIP_TRY(hipGetLastError());
  }
  const int n = nrep * L.n;
  hipLaunchKernelGGL(k_cluster_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, totals(), reinterpret_cast<long long*>(store_slot(this)), n);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_cluster_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels, int side, int connectivity, int every,
                         long long capacity, bflbm_cluster** out) {
  if (!c || !levels || !out) return fail("bflbm_cluster_create: null argument");
  return cluster_create(c, nullptr, source, var, nlevels, levels, side, connectivity, every, capacity, out);
}
int bflbm_batch_cluster_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int connectivity, int every,
                               long long capacity, bflbm_cluster** out) {
  if (!b || !levels || !out) return fail("bflbm_batch_cluster_create: null argument");
  return cluster_create(nullptr, b, source, var, nlevels, levels, side, connectivity, every, capacity, out);
}

int bflbm_cluster_destroy(bflbm_cluster* t) { return store_destroy(t); }
int bflbm_cluster_sample(bflbm_cluster* t) { return store_sample(t, "bflbm_cluster"); }
int bflbm_cluster_reset(bflbm_cluster* t) { return store_reset(t, "bflbm_cluster"); }
int bflbm_cluster_count(const bflbm_cluster* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_cluster", nsamples, nreplicas); }
int bflbm_cluster_read(bflbm_cluster* t, long long first, long long count, long long* counts, long long* steps) {
  return store_read(t, "bflbm_cluster", first, count, reinterpret_cast<double*>(counts), steps);   // 8-byte slots, copied bit for bit
}

int bflbm_cluster_geometry(const bflbm_cluster* t, int* nlevels, int* connectivity, int* brick_x, int* brick_y, int* brick_z, int* bricks, int* launches) {
  if (!t) return fail("bflbm_cluster_geometry: null argument");
  if (nlevels) *nlevels = t->L.n;
  if (connectivity) *connectivity = t->B.conn;
  if (brick_x) *brick_x = cluster_limits::kBx;
  if (brick_y) *brick_y = cluster_limits::kBy;
  if (brick_z) *brick_z = cluster_limits::kBz;
  if (bricks) *bricks = (int)cluster_bricks(t->B.nx, t->B.ny, t->B.nz);
  if (launches) *launches = cluster_limits::kLaunches;
  return 0;
}

int bflbm_cluster_labels(bflbm_cluster* t, int level_index, int* labels) {
  if (!t || !labels) return fail("bflbm_cluster_labels: null argument");
  if (level_index < 0 || level_index >= t->L.n) return fail("bflbm_cluster_labels: level index %d outside 0..%d", level_index, t->L.n - 1);
  if (!recorder_attached(t)) return fail("bflbm_cluster_labels: the owner of the cluster trace was destroyed");
  if (recorder_owner_open(t)) return fail("bflbm_cluster_labels inside an open step");
  HIP_TRY(hipSetDevice(t->device));
  const hipStream_t stream = recorder_stream(t);
  const double* vol;
  long long rep_stride;
  if (t->observe(&vol, &rep_stride)) return 1;
  unsigned long long* caps = t->totals() + t->words();       // the word after the totals: a sample's totals stay as they are
  if (t->label_level(vol, rep_stride, level_index, caps, 0)) return 1;
  const dim3 per_site((unsigned)((t->nsites + 255) / 256), 1, (unsigned)t->nrep);
  hipLaunchKernelGGL(k_cluster_flatten, per_site, dim3(256), 0, stream, t->nsites, t->parent, t->size, caps, 0LL);
  HIP_TRY(hipGetLastError());
  unsigned long long capped = 0;
  HIP_TRY(hipMemcpyAsync(labels, t->size, (size_t)t->nrep * (size_t)t->nsites * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(&capped, caps, sizeof capped, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemsetAsync(caps, 0, sizeof capped, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (capped) return fail("bflbm_cluster_labels: %llu device loops hit their iteration cap", capped);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_CLUSTER_HOST_ONLY

#endif  // BFLBM_CLUSTER_H_
