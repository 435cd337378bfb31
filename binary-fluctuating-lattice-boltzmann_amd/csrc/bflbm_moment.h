// bflbm_moment.h -- moment traces: the box sums of all 19 kinetic moments m = M f of both fluids, of their squares and of
// the products of the two fluids' moments mode by mode, recorded on the device as a time series for a lone single-slab
// context or every replica of a batch (include/bflbm.h, "Moment traces": the definition, the layout of
// a sample and the order of every sum are stated there and only there).  The thermal noise acts on all 19 moments of each
// fluid; every other recorder reads hydrovs, hydrovsbar or the injected noise, so the momentum-flux moments 4..9 and the
// ghost moments 10..18 of the resident state never left d_moments.  Equipartition per mode, the off-diagonal stress of a
// Green-Kubo integral and the co-fluctuation of the two fluids' modes need them; without this a user downloads 38
// populations per site and sample.
// Moments need no gradient stencil and no densities, so the observation and the reduction are one kernel.  A sample is, on
// the owner's stream(s) and without a host synchronisation,
//   k_moment_sums<BATCH>   ONE launch, grid (tiles of a plane, planes, replicas), 256 threads.  A thread takes the 8 turns of
//                          its tile (the profile trace's axis-z tile) one site at a time: pull_site of the resident state
//                          (what populations() returns), d_moments twice, then the 95 accumulators in registers: 38 sums,
//                          38 squares, 19 cross products, every product rounded once and then added.  Every accumulator
//                          has a compile-time index; nothing is picked by selects.  The tree is the lag trace's lag_tree
//                          (levels 128 and 64 through LDS, the rest by lane shifts), 12 accumulators at a time through two
//                          LDS buffers in turn: 95 x 256 doubles at once would be 194 KB.  One partial per (word, tile):
//                          [replica][z][95][tiles].
//   k_moment_finish        grid (95, replicas): the tiles of every plane in tile order from +0.0, then the planes in
//                          sequence z = 0 .. nz-1 from +0.0, straight into the slot [sample][replica][95].
// No ring: there is no bflbm_ring_moment_create.  It would be easy later: k_moment_sums takes a slab by S[cur], Geo and
// own_lo as it takes a lone context, every slab would sum its own planes into [nzl][95][tiles], the ring gather of
// bflbm_recorder.h would bring the blocks to slab 0 and the unchanged k_moment_finish would run there.  It is not built.
// No atomics, no scratch, no grid barrier, nothing of the owner written: not even its scratch state buffer.
// Expected memory traffic per site and sample, derived, not measured: 304 bytes read (38 populations), against the 608 of
// a step; nothing written but 95 x tiles partials per plane.
// What the compiler reports (gfx950, -O3) for k_moment_sums<false> / <true>: see the table at the kernel.  ScratchSize 0
// in both, 49152 bytes of static LDS (tests/test_moment_abi.py reads both from the listing).
// Not built on purpose: variable or pair lists (the record is all of it), per-site output, density-normalised or windowed
// sums, the deviation from the local equilibrium, arbitrary pairs of modes, a source in bflbm_fieldsel.h.
// Host part: plain C++17 that needs a declared int fail(const char*, ...): the layout of a sample, the tile counts, the
// launch shape, the buffers and what a box is refused for.  A stand-alone program defines BFLBM_MOMENT_HOST_ONLY and
// includes it (tests/moment_main.cpp).  HIP part: the lifecycle and the sample store are those of bflbm_recorder.h.
// Included by bflbm.hip after bflbm_lag.h (needs bflbm_ctx, bflbm_batch, BatchRec, pull_site, d_moments,
// lag_tree, batch_sync_table, recorder_refuse_open).
#ifndef BFLBM_MOMENT_H_
#define BFLBM_MOMENT_H_

#include <cstddef>

namespace moment_limits {
constexpr int kModes = 19;                 // the moments of one fluid
constexpr int kWords = 5 * kModes;         // W: sum[38], sq[38], cross[19]
constexpr int kTile = 2048;                // the profile trace's axis-z tile: 256 threads x 8 turns
constexpr int kPerThread = kTile / 256;
constexpr int kSlice = 12;                 // accumulators one call of the tree takes
constexpr int kLdsBytes = 2 * kSlice * 256 * 8;
constexpr int kMaxPlanes = 65535;          // grid.y
constexpr int kMaxReplicas = 65535;        // grid.z
constexpr long long kMaxPlaneSites = (1LL << 31) - 2 * kTile;   // a site of a plane is a 32-bit index, the last tile's turns included
}

namespace {

// the layout of a sample: global moment index i = 19 fluid + a, the numbering of the noise source
inline int moment_word_sum(int fluid, int a) { return moment_limits::kModes * fluid + a; }
inline int moment_word_sq(int fluid, int a) { return 2 * moment_limits::kModes + moment_limits::kModes * fluid + a; }
inline int moment_word_cross(int a) { return 4 * moment_limits::kModes + a; }

// the launch shape and the buffers
inline int moment_tiles(long long plane) { return (int)((plane + moment_limits::kTile - 1) / moment_limits::kTile); }
inline int moment_slices() { return (moment_limits::kWords + moment_limits::kSlice - 1) / moment_limits::kSlice; }
// the partials one plane leaves, and the stage buffer [replica][z][95][tiles], in doubles
inline size_t moment_plane_words(int tiles) { return (size_t)moment_limits::kWords * (size_t)tiles; }
inline size_t moment_stage_words(int nrep, int nz, int tiles) { return (size_t)nrep * (size_t)nz * moment_plane_words(tiles); }

// What every creation call refuses about the owner's box, after the cadence and before any allocation.
int moment_refuse_box(const char* call, int nx, int ny, int nz, int nrep) {
  using namespace moment_limits;
  if (nz > kMaxPlanes) return fail("%s: nz = %d exceeds the %d planes of one launch", call, nz, kMaxPlanes);
  if ((long long)nx * ny > kMaxPlaneSites) return fail("%s: a plane of %lld sites exceeds the %lld of a 32-bit site index", call, (long long)nx * ny, kMaxPlaneSites);
  if (nrep > kMaxReplicas) return fail("%s: %d replicas exceed the %d of one launch", call, nrep, kMaxReplicas);
  return 0;
}

}  // namespace

#ifndef BFLBM_MOMENT_HOST_ONLY

#include <memory>
#include <string>

struct bflbm_moment : bflbm_sample_store {   // d_rec [capacity][nrep][95], d_stage [nrep][nz][95][tiles]
  int nx = 0, ny = 0, nz = 0;
  int tiles = 0;
  bflbm_moment() : bflbm_sample_store("moment trace", "bflbm_moment") {}
  int record() override;
  int finish(hipStream_t stream);
};

namespace {

static_assert(moment_limits::kModes == Q, "the moments of one fluid");

// one site into the 95 accumulators: the moments, their squares, the cross products; the product first, then the sum
__device__ __forceinline__ void moment_add(double (&acc)[moment_limits::kWords], const double (&mf)[Q], const double (&mg)[Q]) {
#pragma unroll
  for (int a = 0; a < Q; ++a) {
    acc[a] += mf[a];
    acc[Q + a] += mg[a];
    const double ff = mf[a] * mf[a], gg = mg[a] * mg[a], fg = mf[a] * mg[a];
    acc[2 * Q + a] += ff;
    acc[3 * Q + a] += gg;
    acc[4 * Q + a] += fg;
  }
}

// grid (tiles of a plane, planes, replicas), 256 threads.  BATCH false: S is the resident buffer S[cur] of a lone context,
// p0 its first own storage plane (own_lo), as k_observe takes them; BATCH true: the replica's
// buffer comes from its record, as k_observe_batch takes it, p0 = 0.  partial: [replica][plane][95][tiles].
// What the compiler reports (gfx950, -O3):
//   BATCH       false   true
//   VGPRs       255     255
//   AGPRs       22      22
//   occupancy   1       1       waves per SIMD (512 registers a wave; 278 in use)
// LDSByteSize 49152 (two buffers of 12 x 256 doubles for the tree) and ScratchSize 0 in both.  The budget: 190 registers
// for the accumulators, which live through the whole loop; the 38 populations (76) die into the 38 moments (76) fluid by
// fluid, so about 90 more are live at the peak.  That is past 256, so one wave per SIMD with some accumulators parked in
// AGPRs between sites; a form below 256 registers would have to split the accumulators over two passes of the loads.
template <bool BATCH>
__global__ void __launch_bounds__(256) k_moment_sums(const double* __restrict__ S0, const BatchRec* __restrict__ recs, int k, Geo G, int p0,
                                                     double* __restrict__ partial) {
  using namespace moment_limits;
  __shared__ double sh[2][kSlice * 256];                   // the per-thread sums on their way into the tree, two buffers in turn
  const int tid = (int)threadIdx.x;
  const int tile = (int)blockIdx.x, tiles = (int)gridDim.x, z = (int)blockIdx.y, rep = (int)blockIdx.z;
  const int plane = G.nx * G.ny;
  const double* __restrict__ S = S0;
  if (BATCH) {
    const BatchRecC R = batch_rec(recs, rep);
    S = R->S[R->cur0 ^ (k & 1)];
  }

  double acc[kWords];
#pragma unroll
  for (int q = 0; q < kWords; ++q) acc[q] = 0.;
#pragma unroll 1
  for (int i = 0; i < kPerThread; ++i) {                   // thread t: the sites t, t + 256, ... of its tile, one at a time
    const int s = tile * kTile + tid + 256 * i;
    if (s < plane) {
      const int y = s / G.nx, x = s - y * G.nx;
      SiteIdx I; site_index(G, x, y, p0 + z, I);
      double fs[Q], gs[Q], mf[Q], mg[Q];
      pull_site(S, G, I, fs, gs);
      d_moments(fs, mf); d_moments(gs, mg);
      moment_add(acc, mf, mg);
    }
  }

  double* __restrict__ out = partial + ((long long)rep * gridDim.y + z) * ((long long)kWords * tiles);
#pragma unroll
  for (int q0 = 0; q0 < kWords; q0 += kSlice) {            // the tree, kSlice accumulators at a time
    const int flip = (q0 / kSlice) & 1;
    const int n = kWords - q0 < kSlice ? kWords - q0 : kSlice;
#pragma unroll
    for (int j = 0; j < kSlice; ++j) if (j < n) sh[flip][j * 256 + tid] = acc[q0 + j];
    lag_tree(sh[flip], n, out + (long long)q0 * tiles, tiles, tile);
  }
}

// grid (95, replicas), 256 threads: word w of the replica's sample.  Thread t adds, starting from +0.0, the tiles of the
// plane z = z0 + t in tile order; thread 0 then adds the planes of the chunk to the running total in sequence, which
// started from +0.0 at z = 0.  partial: [replica][nz][95][tiles]; out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_moment_finish(const double* __restrict__ partial, double* __restrict__ out, int nz, int tiles) {
  using namespace moment_limits;
  __shared__ double planes[256];
  const int t = (int)threadIdx.x, w = (int)blockIdx.x;
  const long long rep = blockIdx.y;
  const double* __restrict__ mine = partial + rep * nz * ((long long)kWords * tiles) + (long long)w * tiles;
  double total = 0.;
  for (int z0 = 0; z0 < nz; z0 += 256) {
    const int z = z0 + t;
    if (z < nz) {
      const double* __restrict__ p = mine + (long long)z * ((long long)kWords * tiles);
      double s = 0.;
      for (int i = 0; i < tiles; ++i) s += p[i];
      planes[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      const int n = nz - z0 < 256 ? nz - z0 : 256;
      for (int i = 0; i < n; ++i) total += planes[i];
    }
    __syncthreads();
  }
  if (t == 0) out[rep * kWords + w] = total;
}

int moment_create(bflbm_ctx* c, bflbm_batch* b, int every, long long capacity, bflbm_moment** out) {
  using namespace moment_limits;
  const char* call = b ? "bflbm_batch_moment_create" : "bflbm_moment_create";
  if (store_refuse_cadence(call, every, capacity)) return 1;
  const int nrep = b ? (int)b->ctx.size() : 1;
  const size_t per = (size_t)nrep * kWords;
  const std::string shape = " x " + std::to_string(kWords) + " words";
  if (store_refuse_capacity(call, capacity, per, nrep, shape.c_str())) return 1;
  if (store_refuse_owner(c, call, "bflbm_batch_moment_create", "moment trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if (moment_refuse_box(call, G.nx, G.ny, G.nz, nrep)) return 1;

  std::unique_ptr<bflbm_moment> t(new bflbm_moment());
  recorder_bind(t.get(), c, b, every);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz;
  t->tiles = moment_tiles((long long)G.nx * G.ny);
  const size_t stage = moment_stage_words(nrep, G.nz, t->tiles);
  if (store_attach(t.get(), c, b, call, every, capacity, per, stage, shape.c_str())) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// the finishing launch into slot n, on the stream that writes the records
int bflbm_moment::finish(hipStream_t stream) {
  hipLaunchKernelGGL(k_moment_finish, dim3((unsigned)moment_limits::kWords, (unsigned)nrep), dim3(256), 0, stream, d_stage, store_slot(this), nz, tiles);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

// enqueue the summing launch and the finishing launch of the resident state into slot n; no host synchronisation
int bflbm_moment::record() {
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const dim3 grid((unsigned)tiles, (unsigned)nz, (unsigned)nrep);
  if (batch) {
    for (const bflbm_ctx* c : batch->ctx) if (c->step_open()) return fail("moment trace sample: a replica has an open step");
    if (batch_sync_table(batch)) return 1;                 // a sample between steps (k = 0 after an init or upload): stale records
    hipLaunchKernelGGL((k_moment_sums<true>), grid, dim3(256), 0, stream, (const double*)nullptr, batch->d_rec, (int)batch->k, batch->G, 0, d_stage);
  } else {
    if (ctx->step_open()) return fail("moment trace sample requested inside an open step");
    hipLaunchKernelGGL((k_moment_sums<false>), grid, dim3(256), 0, stream, ctx->S[ctx->cur], (const BatchRec*)nullptr, 0, ctx->G, own_lo(ctx), d_stage);
  }
  HIP_TRY(hipGetLastError());
  return finish(stream);
}

extern "C" {

int bflbm_moment_create(bflbm_ctx* c, int every, long long capacity, bflbm_moment** out) {
  if (!c || !out) return fail("bflbm_moment_create: null argument");
  return moment_create(c, nullptr, every, capacity, out);
}
int bflbm_batch_moment_create(bflbm_batch* b, int every, long long capacity, bflbm_moment** out) {
  if (!b || !out) return fail("bflbm_batch_moment_create: null argument");
  return moment_create(nullptr, b, every, capacity, out);
}

int bflbm_moment_destroy(bflbm_moment* t) { return store_destroy(t); }
int bflbm_moment_sample(bflbm_moment* t) { return store_sample(t, "bflbm_moment"); }
int bflbm_moment_reset(bflbm_moment* t) { return store_reset(t, "bflbm_moment"); }
int bflbm_moment_count(const bflbm_moment* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_moment", nsamples, nreplicas); }
int bflbm_moment_read(bflbm_moment* t, long long first, long long count, double* sums, long long* steps) {
  return store_read(t, "bflbm_moment", first, count, sums, steps);
}

int bflbm_moment_geometry(const bflbm_moment* t, int* words, int* tile_sites, int* tiles_per_plane) {
  if (!t) return fail("bflbm_moment_geometry: null argument");
  if (words) *words = moment_limits::kWords;
  if (tile_sites) *tile_sites = moment_limits::kTile;
  if (tiles_per_plane) *tiles_per_plane = t->tiles;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_MOMENT_HOST_ONLY

#endif  // BFLBM_MOMENT_H_
