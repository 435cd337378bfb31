// bflbm_coarse.h -- coarse traces: the block sums of chosen hydrovs or hydrovsbar components, and of chosen products of
// them, over a periodic window of the box, recorded on the device as a time series of coarse fields for a lone
// single-slab context or every replica of a batch (include/bflbm.h, "Coarse traces": the rule and the order of every sum
// are stated there and only there).  Every other recorder reduces the fields to numbers; this one keeps them in space:
// with block 1 a slice or a sub-volume, with block 4^3 a 128^3 movie of a 512^3 box at 1/64 of the bytes, with pairs the
// block sums of products and from them the block variances.  Without this a user downloads 22 fields per sample to look at one.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   exactly as the profile and the histogram traces take it (fields_observe),
//   k_coarse_sum<NV>                ONE launch, grid (groups, 1, replicas), 256 threads, which writes the slot
//                                   [sample][replica][q][Z][Y][X] directly: no totals, no finishing launch.
// The summation order of include/bflbm.h (per fine column x of a block C = 0; for dz: for dy: C = C + term; then
// S = 0; for dx: S = S + C(dx)) exists so that the lanes lie along x:
//   a work item                     is (Z, Y, x-tile) of a replica; an x-tile is floor(256 / b_x) b_x fine sites of the
//                                   window, so no block straddles a tile; the last tile of a row may be short.
//   a lane                          owns one fine column of its work item and marches dz, then dy, with four rows' loads in
//                                   flight.  The window is periodic: x, y and z wrap once by a compare and a subtraction.
//                                   Every global load of a wave is a contiguous row segment of 8-byte elements (512 bytes
//                                   for a full wave), or two of them where the wave meets the seam; no lane-strided load.
//                                   A site's variables are loaded once, the pair products are formed in registers, the
//                                   product first and then the add (profile_add of bflbm_profile.h, shared).
//   after the march                 the Q column sums go through LDS once ([Q][256] doubles of dynamic LDS, 2048 Q bytes:
//                                   at most 48 KiB); the first lane of every block adds its b_x columns left to right from
//                                   +0.0 and stores.  With b_x = 1 every lane stores and the row of coarse cells is written
//                                   as one contiguous segment.
// Work items whose tile needs at most 64, 128 lanes share a workgroup: a workgroup takes 256 / L work items at a time,
// L = the lanes of a tile rounded up to whole waves (a 64-site row at block 2: four rows per workgroup), so narrow
// boxes do not idle three waves of four.  Which work items share a workgroup changes no sum: a block belongs to one lane
// group of one work item.  Workgroups per replica: min(ceil(work items / (256 / L)), 2048 / replicas, at least 1); a
// workgroup strides over its turns.
// A block that is large in y and z is marched by ONE lane per column: b_y b_z rows in sequence, and the first lane of a
// block adds up to 256 columns in sequence; blocks are not cut into chunks and there is no merge pass.  The common
// blocks (1 .. 8 per axis) are far from where that hurts; a block of 256 x 256 x 256 is legal and slow.
// Expected memory traffic, derived: 8 nvars bytes read per window site and sample and 8 Q / (b_x b_y b_z) written,
// against the 608 of a step.  Untimed heuristics, not facts (tools/coarse_ab.py times the whole sample, not these): 8-byte
// loads (a lane owns one column, so a 16-byte load would need the two-lane swap of profile_two_turns and an aligned
// row start, which a window origin does not give), the four rows in flight, the 2048 workgroups, the LDS layout [q][lane]
// (the block heads read with stride b_x: bank conflicts for b_x a power of two).
// What the compiler reports (gfx950, -O3), NV = 1 / 3 / 8: 121 / 86 / 141 VGPRs (occupancy 4 / 5 / 3 waves per SIMD;
// NV = 2 is the widest with 170 and occupancy 2: the compiler unrolls the march of the small instantiations further),
// 106 SGPRs in all, LDSByteSize 0 (no static LDS: the column sums are the launch's dynamic LDS) and ScratchSize 0 in all
// eight instantiations (tests/test_coarse_abi.py reads the last two from the listing).
// No ring: a block may straddle two slabs, and gathering field-sized blocks onto slab 0 needs a layout decision of its own;
// there is no bflbm_ring_coarse_create.  Not built on purpose: the noise source, output other than doubles, b_x > 256,
// a merge pass for tall blocks.
// Host part: plain C++17 that needs a declared int fail(const char*, ...); a stand-alone program defines
// BFLBM_COARSE_HOST_ONLY and includes it alone (tests/coarse_main.cpp).  HIP part: the lifecycle and the sample store
// are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by bflbm.hip after bflbm_fieldsel.h,
// bflbm_recorder.h and bflbm_profile.h (needs bflbm_ctx, bflbm_batch, FieldSelection, FstatVars, FstatPairs,
// fields_observe, field_dispatch_nv, profile_add).
#ifndef BFLBM_COARSE_H_
#define BFLBM_COARSE_H_

#include <algorithm>

namespace coarse_limits {
constexpr int kThreads = 256;                            // a workgroup; also the largest b_x
constexpr int kGroups = 2048;                            // workgroups of a launch over all replicas (eight per CU of 256)
constexpr int kInFlight = 4;                             // rows of a marching lane in flight
constexpr long long kMaxItems = 1LL << 30;               // work items of a replica: an int, with room for a turn past the end
}

// the window, the blocks and the launch shape; a by-value kernel parameter
struct CoarseGeo {
  int n[3];                          // the box, x y z
  int o[3], w[3], b[3], c[3];        // origin, extent, block, coarse cells c_a = w_a / b_a
  int tile;                          // fine sites of an x-tile: floor(256 / b_x) b_x
  int ntiles;                        // x-tiles of a window row
  int lanes;                         // L: the lanes a work item takes, min(tile, w_x) rounded up to whole waves
  int share;                         // work items a workgroup takes at a time: 256 / L
  int items;                         // work items of a replica: c_z c_y ntiles
};

namespace {

// What every creation call refuses about its window and its block, in the order of include/bflbm.h.  n, origin, extent,
// block: x y z.
int coarse_refuse_window(const char* call, const int n[3], const int origin[3], const int extent[3], const int block[3]) {
  using namespace coarse_limits;
  static const char axis[3] = {'x', 'y', 'z'};
  for (int a = 0; a < 3; ++a)
    if (origin[a] < 0 || origin[a] >= n[a]) return fail("%s: origin[%c] = %d outside 0..%d", call, axis[a], origin[a], n[a] - 1);
  for (int a = 0; a < 3; ++a)
    if (extent[a] < 1 || extent[a] > n[a]) return fail("%s: extent[%c] = %d outside 1..%d", call, axis[a], extent[a], n[a]);
  for (int a = 0; a < 3; ++a) {
    if (block[a] < 1) return fail("%s: block[%c] must be >= 1 (got %d)", call, axis[a], block[a]);
    if (extent[a] % block[a]) return fail("%s: block[%c] = %d does not divide the extent %d", call, axis[a], block[a], extent[a]);
  }
  if (block[0] > kThreads) return fail("%s: block[x] = %d exceeds %d", call, block[0], kThreads);
  return 0;
}

// the launch shape of an accepted window; items above kMaxItems are left to the caller to refuse (coarse_items)
inline int coarse_tile(int bx) { return coarse_limits::kThreads / bx * bx; }
inline int coarse_tiles(int wx, int bx) { return (wx + coarse_tile(bx) - 1) / coarse_tile(bx); }
inline int coarse_lanes(int wx, int bx) { return (std::min(coarse_tile(bx), wx) + 63) / 64 * 64; }
inline long long coarse_items(const int extent[3], const int block[3]) {
  return (long long)(extent[2] / block[2]) * (extent[1] / block[1]) * coarse_tiles(extent[0], block[0]);
}
// workgroups per replica: a workgroup takes `share` work items at a time and strides over its turns
inline int coarse_groups(long long items, int share, int nrep) {
  const long long turns = (items + share - 1) / share;
  return (int)std::min<long long>(turns, std::max(1, coarse_limits::kGroups / nrep));
}

CoarseGeo coarse_geo(const int n[3], const int origin[3], const int extent[3], const int block[3]) {
  CoarseGeo g;
  for (int a = 0; a < 3; ++a) { g.n[a] = n[a]; g.o[a] = origin[a]; g.w[a] = extent[a]; g.b[a] = block[a]; g.c[a] = extent[a] / block[a]; }
  g.tile = coarse_tile(block[0]);
  g.ntiles = coarse_tiles(extent[0], block[0]);
  g.lanes = coarse_lanes(extent[0], block[0]);
  g.share = coarse_limits::kThreads / g.lanes;
  g.items = (int)std::min(coarse_items(extent, block), coarse_limits::kMaxItems);
  return g;
}

}  // namespace

#ifndef BFLBM_COARSE_HOST_ONLY

#include <memory>
#include <string>

struct bflbm_coarse : bflbm_sample_store {   // d_rec [capacity][nrep][nq][cz][cy][cx]; no stage buffer
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar
  int nq = 0;                       // nq = nvars + npairs
  FstatPairs pairs;
  CoarseGeo G;
  double* fields = nullptr;         // a batch: [nrep][nvars][nsites]
  bflbm_coarse() : bflbm_sample_store("coarse trace", "bflbm_coarse") {}
  ~bflbm_coarse() override {
    if (fields) { hipSetDevice(device); hipFree(fields); }
  }
  int record() override;
};

namespace {

// grid (groups, 1, replicas), 256 threads, 2048 nq bytes of dynamic LDS.  fields: the dense volumes, variable v of
// replica r at fields + r rep_stride + V.vol[v] comp_stride, [nz][ny][nx]; out: the slot, [replica][nq][cz][cy][cx].
// NV, the number of variables, is a template parameter: the site values and the accumulators are register arrays.
template <int NV>
__global__ void __launch_bounds__(256) k_coarse_sum(const double* __restrict__ fields, long long rep_stride, long long comp_stride,
                                                    double* __restrict__ out, CoarseGeo G, FstatVars V, FstatPairs P) {
  using namespace coarse_limits;
  constexpr int NQ = NV + profile_limits::kMaxPairs;
  extern __shared__ double coarse_sh[];                   // [nq][256]
  const int tid = (int)threadIdx.x, nq = NV + P.n;
  const int sub = tid / G.lanes, t = tid - sub * G.lanes; // which of the workgroup's work items, and the lane within it
  const long long plane = (long long)G.n[0] * G.n[1];
  const double* vol[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) vol[v] = fields + (long long)blockIdx.z * rep_stride + (long long)V.vol[v] * comp_stride;
  double* __restrict__ mine = out + (long long)blockIdx.z * nq * G.c[2] * G.c[1] * G.c[0];
  const int rows = G.b[2] * G.b[1];                       // the rows a lane marches: dz slow, dy fast

  const int turns = (G.items + G.share - 1) / G.share;
  for (int turn = (int)blockIdx.x; turn < turns; turn += (int)gridDim.x) {
    const int item = turn * G.share + sub;
    const int zy = item / G.ntiles, tile = item - zy * G.ntiles;
    const int Z = zy / G.c[1], Y = zy - Z * G.c[1];
    const int xi = tile * G.tile + t;                     // the fine column within the window
    const bool in = sub < G.share && item < G.items && t < G.tile && xi < G.w[0];
    double acc[NQ][1];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q][0] = 0.;
    if (in) {
      int x = G.o[0] + xi;
      if (x >= G.n[0]) x -= G.n[0];
      const int z0 = G.o[2] + Z * G.b[2], y0 = G.o[1] + Y * G.b[1];
      // row m of the march is (dz, dy) = (m / b_y, m % b_y); its offset in a volume
      auto row_at = [&](int m) {
        const int dz = m / G.b[1], dy = m - dz * G.b[1];
        int z = z0 + dz, y = y0 + dy;
        if (z >= G.n[2]) z -= G.n[2];
        if (y >= G.n[1]) y -= G.n[1];
        return (long long)z * plane + (long long)y * G.n[0] + x;
      };
      int m = 0;
      for (; m + kInFlight <= rows; m += kInFlight) {
        double x0[kInFlight][NV][1];
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) {
          const long long at = row_at(m + j);
#pragma unroll
          for (int v = 0; v < NV; ++v) x0[j][v][0] = vol[v][at];
        }
#pragma unroll
        for (int j = 0; j < kInFlight; ++j) profile_add<NV, 1>(acc, x0[j], P);
      }
      for (; m < rows; ++m) {
        const long long at = row_at(m);
        double x0[NV][1];
#pragma unroll
        for (int v = 0; v < NV; ++v) x0[v][0] = vol[v][at];
        profile_add<NV, 1>(acc, x0, P);
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) if (q < nq) coarse_sh[q * kThreads + tid] = acc[q][0];
    }
    __syncthreads();
    if (in && t % G.b[0] == 0) {                           // the first lane of a block: its b_x columns left to right
      const long long cell = ((long long)Z * G.c[1] + Y) * G.c[0] + xi / G.b[0];
      const long long cells = (long long)G.c[2] * G.c[1] * G.c[0];
      for (int q = 0; q < nq; ++q) {
        const double* __restrict__ col = coarse_sh + q * kThreads + tid;
        double s = 0.;
        for (int dx = 0; dx < G.b[0]; ++dx) s += col[dx];
        mine[q * cells + cell] = s;
      }
    }
    __syncthreads();                                      // the next turn overwrites the column sums
  }
}

int coarse_create(bflbm_ctx* c, bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                  const int* origin, const int* extent, const int* block, int every, long long capacity, bflbm_coarse** out) {
  const char* call = b ? "bflbm_batch_coarse_create" : "bflbm_coarse_create";
  if (field_refuse_args(call, source, 1, nvars, vars, npairs, pair_a, pair_b)) return 1;
  const Geo& G = c ? c->G : b->G;
  const int n[3] = {G.nx, G.ny, G.nz};
  if (coarse_refuse_window(call, n, origin, extent, block)) return 1;
  if (coarse_items(extent, block) > coarse_limits::kMaxItems)
    return fail("%s: %lld work items per replica exceed %lld", call, coarse_items(extent, block), coarse_limits::kMaxItems);
  if (store_refuse_owner(c, call, "bflbm_batch_coarse_create", "coarse trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  if (store_refuse_cadence(call, every, capacity)) return 1;

  std::unique_ptr<bflbm_coarse> t(new bflbm_coarse());
  recorder_bind(t.get(), c, b, every);
  t->nsites = (long long)G.nx * G.ny * G.nz;
  t->nq = nvars + npairs;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  t->pairs = field_pairs(npairs, pair_a, pair_b);
  t->G = coarse_geo(n, origin, extent, block);

  const size_t per = (size_t)t->nrep * t->nq * t->G.c[2] * t->G.c[1] * t->G.c[0];
  const std::string shape = " x " + std::to_string(t->nq) + " sums x " + std::to_string(t->G.c[2]) + " x " + std::to_string(t->G.c[1]) + " x "
                            + std::to_string(t->G.c[0]) + " blocks";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the fields of a batch
  const size_t fb = b ? (size_t)t->nrep * nvars * (size_t)t->nsites * sizeof(double) : 0;
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu bytes; then records %zu x %lld): %s", call, fb, per * sizeof(double), capacity,
                hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, 1, shape.c_str())) return 1;      // a stage buffer of one unused double
  *out = t.release();
  return 0;
}

}  // namespace

// enqueue the observation and the one summing launch of the resident state into slot n; no host synchronisation
int bflbm_coarse::record() {
  using namespace coarse_limits;
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "coarse trace sample", &dense, &rep_stride)) return 1;
  const dim3 grid((unsigned)coarse_groups(G.items, G.share, nrep), 1, (unsigned)nrep);
  const size_t lds = (size_t)nq * kThreads * sizeof(double);
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_coarse_sum<decltype(nv)::value>), grid, dim3(kThreads), lds, stream, dense, rep_stride, nsites, store_slot(this), G,
                           fs.vol, pairs);
      })) return fail("coarse trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_coarse_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                        const int* origin, const int* extent, const int* block, int every, long long capacity, bflbm_coarse** out) {
  if (!c || !vars || !origin || !extent || !block || !out) return fail("bflbm_coarse_create: null argument");
  return coarse_create(c, nullptr, source, nvars, vars, npairs, pair_a, pair_b, origin, extent, block, every, capacity, out);
}
int bflbm_batch_coarse_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                              const int* origin, const int* extent, const int* block, int every, long long capacity, bflbm_coarse** out) {
  if (!b || !vars || !origin || !extent || !block || !out) return fail("bflbm_batch_coarse_create: null argument");
  return coarse_create(nullptr, b, source, nvars, vars, npairs, pair_a, pair_b, origin, extent, block, every, capacity, out);
}

int bflbm_coarse_destroy(bflbm_coarse* t) { return store_destroy(t); }
int bflbm_coarse_sample(bflbm_coarse* t) { return store_sample(t, "bflbm_coarse"); }
int bflbm_coarse_reset(bflbm_coarse* t) { return store_reset(t, "bflbm_coarse"); }
int bflbm_coarse_count(const bflbm_coarse* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_coarse", nsamples, nreplicas); }
int bflbm_coarse_read(bflbm_coarse* t, long long first, long long count, double* sums, long long* steps) {
  return store_read(t, "bflbm_coarse", first, count, sums, steps);
}

int bflbm_coarse_geometry(const bflbm_coarse* t, int* cx, int* cy, int* cz, int* nsums, int* tile_sites, int* items, int* groups) {
  if (!t) return fail("bflbm_coarse_geometry: null argument");
  if (cx) *cx = t->G.c[0];
  if (cy) *cy = t->G.c[1];
  if (cz) *cz = t->G.c[2];
  if (nsums) *nsums = t->nq;
  if (tile_sites) *tile_sites = t->G.tile;
  if (items) *items = t->G.items;
  if (groups) *groups = coarse_groups(t->G.items, t->G.share, t->nrep) * t->nrep;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_COARSE_HOST_ONLY

#endif  // BFLBM_COARSE_H_
