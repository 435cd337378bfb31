// bflbm_morph.h -- morphology traces: the four Minkowski functionals (volume, interface area, mean breadth, Euler
// characteristic) of the set {v >= level} or {v < level} of one observed hydrovs or hydrovsbar variable at 1 to 8 levels,
// recorded on the device as a time series of 64-bit integer counts for a lone single-slab context or every replica of a
// batch (include/bflbm.h, "Morphology traces": the counting rule and the layout of a sample are stated there and only
// there).  How much interface a coarsening mixture has (L = V / S), whether it is bicontinuous or has broken into
// droplets (the sign of chi) and how many droplets there are (chi itself) are questions about the shape of the domains;
// without this a user downloads the field per sample and counts on the host.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   of the one variable, exactly as the histogram trace takes it (fields_observe),
//   k_morph_count<NL>               the counting launch, grid (work items, 1, replicas), 256 threads, one work item per
//                                   workgroup: a tile of 1024 consecutive plane sites p = y nx + x (a thread takes the
//                                   four sites tid + 256 k) times a chunk of Zc planes.  A thread marches its sites
//                                   along z.  Per plane it loads a site's value and the values of its x+, y+ and x+y+
//                                   neighbours (the wraps inside the row and inside the plane are four offsets computed
//                                   once), forms each value's 8-bit level mask and from them the OR-masks of the
//                                   (x,x+), (y,y+) and (x,x+,y,y+) neighbourhoods, four bytes of one register.  The
//                                   register of the previous plane is kept, so a cell between the planes z and z+ costs
//                                   one new plane; the last chunk's z+ wraps to plane 0.  Per level and counter one
//                                   __popcll(__ballot(bit)) is added into a wave-uniform 32-bit counter: no per-lane
//                                   counters, no cross-lane reduction.  After the march one LDS add per wave and
//                                   counter, then one 64-bit global add per non-zero counter and workgroup into
//                                   totals [replica][nlevels][4], as the histogram trace does,
//   k_hist_finish                   the histogram trace's finishing launch, shared: the totals into the slot
//                                   [sample][replica][nlevels][4], and the totals back to zero for the next sample.
// Integer sums commute, so the record is exact whatever the launch geometry.
// Neighbours by cached re-loads, not LDS masks: the x+ value lies in the same 128-byte line for 15 lanes of 16 and the
// y+ row is the next turn's own row for three turns of four where a tile spans rows; the re-loads cost address and
// cache bandwidth and no memory traffic, and the kernel needs no halo staging, no barrier in the march and no second
// code path for planes narrower than a tile.  Expected memory traffic, derived: every plane site of a chunk is fetched
// once for Zc + 1 planes, 8 (Zc + 1) / Zc bytes per site, plus the one row of nx sites past the tile's end that the y+
// re-loads touch and the next tile fetches too, 8 nx / 1024 bytes per site where the caches do not hold it between the
// two workgroups: at 256^3, where Zc = 16, 8.5 + 2 = 10.5 bytes per site against the 608 of a step.
// A workgroup meets 1024 Zc <= 65536 cells and a cell adds at most 3 to a counter (three faces, three edges), so no
// 32-bit counter passes 196608: the bound that keeps them from wrapping, as hist_limits states its own.
// The level count is a template parameter, NL = 1 .. 8, compiled once each: the 4 NL counters are wave-uniform and live
// in scalar registers, which only static indices reach; a runtime loop over the levels would put them into LDS or
// per-lane registers.  The side is a runtime value: one exclusive-or of a mask with a uniform word.
// Zc: the largest of 64, 32, 16, 8 that leaves 1024 work items over all replicas (four workgroups per CU of 256), else
// 8, and never more than nz.  The tile and this rule are untimed heuristics.
// No ring: a cell crosses the slab boundary and needs the next slab's first observed plane, which no slab holds; there
// is no bflbm_ring_morph_create (the interface trace's exclusion).
// Host part: plain C++17 that needs bflbm_fieldsel.h's host part and a declared int fail(const char*, ...): the argument
// refusals, the levels and the launch shape.  A stand-alone program defines BFLBM_MORPH_HOST_ONLY (and
// BFLBM_FIELDSEL_HOST_ONLY) and includes it after bflbm_fieldsel.h (tests/morph_main.cpp).  HIP part: the lifecycle and
// the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by bflbm.hip after
// bflbm_hist.h (needs bflbm_ctx, bflbm_batch, FieldSelection, fields_observe, field_dispatch_nv, k_hist_finish).
#ifndef BFLBM_MORPH_H_
#define BFLBM_MORPH_H_

#include <algorithm>
#include <cmath>

namespace morph_limits {
constexpr int kMaxLevels = 8;
constexpr int kSitesPerThread = 4;
constexpr int kTile = 256 * kSitesPerThread;   // plane sites of a work item
constexpr int kMinChunk = 8, kMaxChunk = 64;   // planes of a work item
constexpr long long kWantItems = 1024;         // work items over all replicas that the chunk is shortened for
constexpr long long kMaxPlane = 1LL << 30;     // plane sites: in-plane offsets are 32-bit
static_assert(3LL * kTile * kMaxChunk < (1LL << 32), "a cell adds at most 3 to a counter: 32 bits hold a workgroup's cells");
static_assert(kMaxLevels <= fstat_limits::kMaxVars, "field_dispatch_nv picks the instantiation");
}

// the levels and the side; a by-value kernel parameter
struct MorphLevels {
  int n, side;                       // side 0: a site is occupied where v >= t, side 1: where v < t; a NaN nowhere
  double t[morph_limits::kMaxLevels];
};

namespace {

// What every creation call refuses about its levels, side, source and variable, in the order of include/bflbm.h.
int morph_refuse_args(const char* call, int source, int var, int nlevels, const double* levels, int side) {
  using namespace morph_limits;
  if (nlevels < 1 || nlevels > kMaxLevels) return fail("%s: 1..%d levels (got %d)", call, kMaxLevels, nlevels);
  if (!levels) return fail("%s: null argument", call);
  for (int l = 0; l < nlevels; ++l)
    if (!std::isfinite(levels[l])) return fail("%s: level %d is not finite (got %g)", call, l, levels[l]);
  if (side != 0 && side != 1) return fail("%s: side must be 0 (v >= level) or 1 (v < level) (got %d)", call, side);
  return field_refuse_args(call, source, 1, 1, &var, 0, nullptr, nullptr);
}

// the levels of accepted arguments
MorphLevels morph_levels(int nlevels, const double* levels, int side) {
  MorphLevels L;
  L.n = nlevels; L.side = side;
  for (int l = 0; l < morph_limits::kMaxLevels; ++l) L.t[l] = l < nlevels ? levels[l] : 0.;
  return L;
}

// the launch shape over a box of `plane` sites per plane and nz planes, for each of nrep replicas
inline long long morph_tiles(long long plane) { return (plane + morph_limits::kTile - 1) / morph_limits::kTile; }
inline int morph_chunks(int nz, int zc) { return (nz + zc - 1) / zc; }
inline int morph_chunk(long long plane, int nz, int nrep) {
  using namespace morph_limits;
  int zc = kMaxChunk;
  while (zc > kMinChunk && morph_tiles(plane) * morph_chunks(nz, zc) * nrep < kWantItems) zc /= 2;
  return std::min(zc, nz);
}
inline long long morph_items(long long plane, int nz, int nrep) { return morph_tiles(plane) * morph_chunks(nz, morph_chunk(plane, nz, nrep)); }

}  // namespace

#ifndef BFLBM_MORPH_HOST_ONLY

#include <memory>
#include <string>

struct bflbm_morph : bflbm_sample_store {    // d_rec [capacity][nrep][nlevels][4] as long long, d_stage: the totals [nrep][nlevels][4]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar; one variable
  MorphLevels L;
  double* fields = nullptr;         // a batch: [nrep][nsites]
  bflbm_morph() : bflbm_sample_store("morphology trace", "bflbm_morph") {}
  ~bflbm_morph() override {
    if (fields) { hipSetDevice(device); hipFree(fields); }
  }
  unsigned long long* totals() const { return reinterpret_cast<unsigned long long*>(d_stage); }
  int record() override;
};

namespace {

// bit l: the value occupies its site at level l.  v < t is "not v >= t, and v is a number" for a finite t, so side 1 is the
// complement of side 0 within the NL bits (flip: those bits for side 1, else 0) and a NaN clears both: no branch on the side
template <int NL> __device__ __forceinline__ unsigned morph_mask(double v, const MorphLevels& L, unsigned flip) {
  unsigned m = 0u;
#pragma unroll
  for (int l = 0; l < NL; ++l) m |= v >= L.t[l] ? 1u << l : 0u;
  return v == v ? m ^ flip : 0u;
}

// the sites of the wave's lanes whose bit is set
__device__ __forceinline__ unsigned morph_votes(unsigned bit) { return (unsigned)__popcll(__ballot((int)(bit & 1u))); }

// grid (tiles per plane x chunks, 1, replicas), 256 threads.  field: the dense volume [nz][ny][nx] of replica r at
// field + r rep_stride; totals: [replica][NL][4] = N3, N2, N1, N0 per level.
template <int NL>
__global__ void __launch_bounds__(256) k_morph_count(const double* __restrict__ field, long long rep_stride, int nx, int ny, int nz, int zc,
                                                     unsigned long long* __restrict__ totals, MorphLevels L) {
  using namespace morph_limits;
  __shared__ unsigned sh[4 * kMaxLevels];
  const int tid = (int)threadIdx.x;
  if (tid < 4 * kMaxLevels) sh[tid] = 0u;
  __syncthreads();
  const int plane = nx * ny;
  const int tiles = (plane + kTile - 1) / kTile;
  const int tile = (int)blockIdx.x % tiles, chunk = (int)blockIdx.x / tiles;
  const double* __restrict__ vol = field + (long long)blockIdx.z * rep_stride;

  // a site's own offset in the plane and those of its x+, y+ and x+y+ neighbours, wrapped; a site past the plane reads
  // site 0 and its masks are zeroed
  int at[kSitesPerThread][4];
  bool in[kSitesPerThread];
#pragma unroll
  for (int k = 0; k < kSitesPerThread; ++k) {
    const int p = tile * kTile + k * 256 + tid;
    in[k] = p < plane;
    const int pc = in[k] ? p : 0;
    const int y = pc / nx, x = pc - y * nx;
    const int px = x + 1 < nx ? pc + 1 : pc + 1 - nx;
    const int dy = y + 1 < ny ? nx : nx - plane;
    at[k][0] = pc; at[k][1] = px; at[k][2] = pc + dy; at[k][3] = px + dy;
  }
  const unsigned flip = L.side ? (1u << NL) - 1u : 0u;
  // byte 0: the site's mask, byte 1: OR over (x, x+), byte 2: over (y, y+), byte 3: over (x, x+, y, y+), of plane z
  auto plane_masks = [&](int z, int k) -> unsigned {
    const double* __restrict__ pl = vol + (long long)z * plane;
    const unsigned m = morph_mask<NL>(pl[at[k][0]], L, flip), mx = m | morph_mask<NL>(pl[at[k][1]], L, flip),
                   my = m | morph_mask<NL>(pl[at[k][2]], L, flip), mxy = mx | my | morph_mask<NL>(pl[at[k][3]], L, flip);
    return in[k] ? (m | (mx << 8) | (my << 16) | (mxy << 24)) : 0u;
  };

  const int z0 = chunk * zc, z1 = min(nz, z0 + zc);
  unsigned prev[kSitesPerThread];
#pragma unroll
  for (int k = 0; k < kSitesPerThread; ++k) prev[k] = plane_masks(z0, k);
  unsigned cnt[NL][4];
#pragma unroll
  for (int l = 0; l < NL; ++l) { cnt[l][0] = 0u; cnt[l][1] = 0u; cnt[l][2] = 0u; cnt[l][3] = 0u; }
  for (int z = z0; z < z1; ++z) {
    const int zn = z + 1 == nz ? 0 : z + 1;
    unsigned next[kSitesPerThread];
#pragma unroll
    for (int k = 0; k < kSitesPerThread; ++k) next[k] = plane_masks(zn, k);
#pragma unroll
    for (int k = 0; k < kSitesPerThread; ++k) {
      const unsigned a = prev[k], o = a | next[k];            // o: the same neighbourhoods over the planes z and z+
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        cnt[l][0] += morph_votes(a >> l);                                                            // the cube
        cnt[l][1] += morph_votes(a >> (8 + l)) + morph_votes(a >> (16 + l)) + morph_votes(o >> l);   // the faces across x, y, z
        cnt[l][2] += morph_votes(o >> (16 + l)) + morph_votes(o >> (8 + l)) + morph_votes(a >> (24 + l));   // the edges along x, y, z
        cnt[l][3] += morph_votes(o >> (24 + l));                                                     // the vertex
      }
      prev[k] = next[k];
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cnt[l][j]) atomicAdd(&sh[4 * l + j], cnt[l][j]);
  }
  __syncthreads();
  if (tid < 4 * NL) {
    const unsigned n = sh[tid];
    if (n) atomicAdd(&totals[(long long)blockIdx.z * (4 * NL) + tid], (unsigned long long)n);
  }
}

int morph_create(bflbm_ctx* c, bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int every,
                 long long capacity, bflbm_morph** out) {
  const char* call = b ? "bflbm_batch_morph_create" : "bflbm_morph_create";
  if (morph_refuse_args(call, source, var, nlevels, levels, side)) return 1;
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_morph_create", "morphology trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if ((long long)G.nx * G.ny > morph_limits::kMaxPlane)
    return fail("%s: a plane of %lld sites exceeds %lld", call, (long long)G.nx * G.ny, morph_limits::kMaxPlane);

  std::unique_ptr<bflbm_morph> t(new bflbm_morph());
  recorder_bind(t.get(), c, b, every);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->fs = field_select(b != nullptr, source, 1, &var);
  t->L = morph_levels(nlevels, levels, side);

  const size_t per = (size_t)t->nrep * nlevels * 4;
  const std::string shape = " x " + std::to_string(nlevels) + " levels x 4 counts";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the field of a batch
  const size_t sb = per * sizeof(long long);
  const size_t fb = b ? (size_t)t->nrep * (size_t)t->nsites * sizeof(double) : 0;
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (field %zu bytes; then records %zu x %lld + totals %zu): %s", call, fb, sb, capacity, sb, hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, per, shape.c_str())) return 1;
  // The totals are the store's stage buffer, so their zeroing comes after the owner's list took the trace: its failure
  // detaches again (store_destroy), as the histogram trace's does.
  bflbm_morph* m = t.release();
  e = hipMemsetAsync(m->d_stage, 0, sb, recorder_stream(m));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(m);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = m;
  return 0;
}

}  // namespace

// enqueue the observation, the counting and the finishing launch of the resident state into slot n; no host synchronisation
int bflbm_morph::record() {
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "morphology trace sample", &dense, &rep_stride)) return 1;
  const double* vol = dense + (long long)fs.vol.vol[0] * nsites;
  const long long plane = (long long)nx * ny;
  const int zc = morph_chunk(plane, nz, nrep);
  const dim3 grid((unsigned)morph_items(plane, nz, nrep), 1, (unsigned)nrep);
  if (!field_dispatch_nv(L.n, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        hipLaunchKernelGGL((k_morph_count<NL>), grid, dim3(256), 0, stream, vol, rep_stride, nx, ny, nz, zc, totals(), L);
      })) return fail("morphology trace: %d levels", L.n);
  HIP_TRY(hipGetLastError());
  const int n = nrep * L.n * 4;
  hipLaunchKernelGGL(k_hist_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     totals(), reinterpret_cast<long long*>(store_slot(this)), n, (const long long*)nullptr, 0);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_morph_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels, int side, int every, long long capacity,
                       bflbm_morph** out) {
  if (!c || !levels || !out) return fail("bflbm_morph_create: null argument");
  return morph_create(c, nullptr, source, var, nlevels, levels, side, every, capacity, out);
}
int bflbm_batch_morph_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int every, long long capacity,
                             bflbm_morph** out) {
  if (!b || !levels || !out) return fail("bflbm_batch_morph_create: null argument");
  return morph_create(nullptr, b, source, var, nlevels, levels, side, every, capacity, out);
}

int bflbm_morph_destroy(bflbm_morph* t) { return store_destroy(t); }
int bflbm_morph_sample(bflbm_morph* t) { return store_sample(t, "bflbm_morph"); }
int bflbm_morph_reset(bflbm_morph* t) { return store_reset(t, "bflbm_morph"); }
int bflbm_morph_count(const bflbm_morph* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_morph", nsamples, nreplicas); }
int bflbm_morph_read(bflbm_morph* t, long long first, long long count, long long* counts, long long* steps) {
  return store_read(t, "bflbm_morph", first, count, reinterpret_cast<double*>(counts), steps);   // 8-byte slots, copied bit for bit
}

int bflbm_morph_geometry(const bflbm_morph* t, int* nlevels, int* tile_sites, int* chunk_planes, int* items, int* groups) {
  if (!t) return fail("bflbm_morph_geometry: null argument");
  const long long plane = (long long)t->nx * t->ny;
  const long long n = morph_items(plane, t->nz, t->nrep);
  if (nlevels) *nlevels = t->L.n;
  if (tile_sites) *tile_sites = morph_limits::kTile;
  if (chunk_planes) *chunk_planes = morph_chunk(plane, t->nz, t->nrep);
  if (items) *items = (int)n;
  if (groups) *groups = (int)(n * t->nrep);                // one work item per workgroup: the launch does not stride
  return 0;
}

}  // extern "C"

#endif  // BFLBM_MORPH_HOST_ONLY

#endif  // BFLBM_MORPH_H_
