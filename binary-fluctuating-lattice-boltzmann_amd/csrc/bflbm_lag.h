// bflbm_lag.h -- lag traces: two-time correlations of chosen hydrovs or hydrovsbar components against time origins kept on
// the device, recorded as a time series for a lone single-slab context or every replica of a batch (include/bflbm.h,
// "Lag traces": the origin schedule, the layout of a sample, the persistence rule and the order of every sum are stated
// there and only there).  Every other recorder reduces the fields of ONE instant; the velocity autocorrelation
// sum_x u(x, t0 + lag) . u(x, t0) of an equilibrium run, the two-time function C(t, t_w) = sum_x phi(x, t) phi(x, t_w) and
// the persistence P(t, t_w) of a quench need two.  Without this a user downloads hydrovs per sample and keeps the frames.
// The trace keeps R origins [replica][slot][variable][site] and, with persistence, one 16-bit mask per site.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   exactly as the profile trace takes it (fields_observe),
//   k_lag_label                     only at a sample that takes an origin: the owner's step counters into the slot's label,
//   k_lag_products<NV>              ONE launch, grid (tiles of a plane, planes, replicas), 256 threads.  A thread loads the
//                                   current values of its 8 turns of the profile trace's axis-z tile once (profile_two_turns:
//                                   16-byte loads where the plane is aligned) and keeps them in registers, NV x 8 doubles;
//                                   adds them into now; stores them into the slot that takes an origin; then loops over the
//                                   live slots with the origin's values streaming through: per slot and pair the product
//                                   rounded once and added, one per-thread sum, the tree, one partial per (plane, tile,
//                                   slot, pair).  The slot taken at this sample uses the registers, not the memory just
//                                   written.  With persistence the thread loads its sites' masks once, updates every live
//                                   bit from the values in registers and stores them; the set bits are counted by wave
//                                   ballots into a wave-uniform counter, one LDS add per wave and slot, one 64-bit global
//                                   add per non-zero counter and workgroup (the histogram trace's scheme; integers commute).
//   k_lag_planes                    the tiles of every plane in tile order,
//   k_lag_finish                    the planes in sequence z = 0 .. nz-1 from +0.0, the counters and the labels into the slot
//                                   [sample][replica][W], the counters back to zero.
// No atomics on doubles, no scratch, no grid barrier.  The tree is profile_plane_z's (levels 128 and 64 through LDS, the rest
// by lane shifts in wave 0), restated here as the device function lag_tree because there it is part of the plane's body;
// no existing kernel gains an instantiation.  A pair loads the origin variable b by its own pointer: pairs that share b
// read it again through the cache, which the derived traffic below does not count.
// Expected memory traffic per site and sample, derived, not measured: 8 nvars (1 + L) bytes read, L the live slots,
// 8 nvars bytes written at an origin sample, 4 bytes for the mask (2 read, 2 written).  With three velocity components and
// 16 origins that is 408 bytes, against the 608 of a step.  Measured (tools/lag_ab.py, profiles/lag_throughput.txt): the
// launch reaches 3.85 TB/s on these bytes at 256^3 with NV = 4 and 8 origins, 3.63 TB/s on 16 x 64^3; not tuned.
// What the compiler reports (gfx950, -O3), NV = 1 / 3 / 8: 82 / 125 / 213 VGPRs, occupancy 4 / 4 / 2 waves per SIMD, no
// AGPRs, 32832 bytes of static LDS and ScratchSize 0 (the table at k_lag_products has all eight).  A first form that kept
// the sums of all 8 pairs of a slot in registers and unrolled the pairs took 256 VGPRs + 256 AGPRs and spilled in seven
// instantiations; the shipped form takes one pair at a time (8 doubles of the origin in flight per thread) and hands
// the per-thread sums to the tree through LDS.
// No ring: there is no bflbm_ring_lag_create.  It would be easy later: the origins and the masks are per-site data that stay
// on the slab that owns the site, and the partials gather in plane order exactly as the profile trace's do (the ring gather
// of bflbm_recorder.h); the integer counters add.  It is not built.  Not built on purpose either: the noise source, more
// than 16 origins, logarithmically spaced origins, per-site lagged products.
// Host part: plain C++17 beside field_select that needs bflbm_fieldsel.h's host part and a declared int fail(const char*,
// ...): the refusals, the layout of a sample, the slot schedule and the launch shape.  A stand-alone program defines
// BFLBM_LAG_HOST_ONLY (and BFLBM_FIELDSEL_HOST_ONLY) and includes it after bflbm_fieldsel.h (tests/lag_main.cpp).  HIP part:
// the lifecycle and the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by
// bflbm.hip after bflbm_profile.h (needs bflbm_ctx, bflbm_batch, FieldSelection, FstatVars, fields_observe,
// field_dispatch_nv, fstat_pick, fstat_aligned, profile_two_turns).
#ifndef BFLBM_LAG_H_
#define BFLBM_LAG_H_

#include <cmath>

namespace lag_limits {
constexpr int kMaxVars = fstat_limits::kMaxVars;
constexpr int kMaxPairs = 8;
constexpr int kMaxOrigins = 16;      // one bit of a site's 16-bit mask per slot
constexpr int kTile = 2048;          // the profile trace's axis-z tile: 256 threads x 8 turns
constexpr int kPerThread = kTile / 256;
constexpr int kMaxPlanes = 65535;    // grid.y
constexpr int kLabelChunk = 32;      // step counters a labelling launch carries by value
}

// what the summing launch needs besides the fields; a by-value kernel parameter
struct LagPlan {
  int R, npairs;
  int pa[lag_limits::kMaxPairs], pb[lag_limits::kMaxPairs];
  int take;                          // the slot that takes an origin at this sample, or -1
  unsigned live;                     // bit r: slot r holds an origin (the one taken now included)
  int pslot;                         // the persistence variable's slot, or -1
  double level;
  int qtot;                          // sums per (plane, tile): nvars + R npairs
};

namespace {

// What every creation call refuses about its arguments, in the order of include/bflbm.h.
int lag_refuse_args(const char* call, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                    int norigins, int origin_stride, int persist_slot, double persist_level) {
  using namespace lag_limits;
  if (source < 0 || source > 1) return fail("%s: source must be 0 (hydrovs) or 1 (hydrovsbar) (got %d)", call, source);
  if (nvars < 1 || nvars > kMaxVars) return fail("%s: 1..%d variables (got %d)", call, kMaxVars, nvars);
  if (npairs < 1 || npairs > kMaxPairs) return fail("%s: 1..%d pairs (got %d)", call, kMaxPairs, npairs);
  if (field_refuse_args(call, source, 1, nvars, vars, npairs, pair_a, pair_b)) return 1;
  if (norigins < 1 || norigins > kMaxOrigins) return fail("%s: 1..%d origins (got %d)", call, kMaxOrigins, norigins);
  if (origin_stride < 1) return fail("%s: origin_stride must be >= 1 (got %d)", call, origin_stride);
  if (persist_slot < -1 || persist_slot >= nvars)
    return fail("%s: persist_slot %d outside -1..%d", call, persist_slot, nvars - 1);
  if (persist_slot >= 0 && !std::isfinite(persist_level)) return fail("%s: persist_level must be finite (got %g)", call, persist_level);
  return 0;
}

// the layout of a sample: W = nvars + R (2 + npairs) 8-byte words per replica
inline int lag_words(int nvars, int npairs, int R) { return nvars + R * (2 + npairs); }
inline int lag_word_origin_step(int nvars, int npairs, int r) { return nvars + r * (2 + npairs); }
inline int lag_word_alive(int nvars, int npairs, int r) { return nvars + r * (2 + npairs) + 1; }
inline int lag_word_corr(int nvars, int npairs, int r, int p) { return nvars + r * (2 + npairs) + 2 + p; }

// the slot schedule: sample n takes an origin when n % E == 0, into slot (n / E) % R
inline int lag_take(long long n, int R, int E) { return n % E == 0 ? (int)((n / E) % R) : -1; }
// the live slots after sample n has taken its origin: the first min(R, n / E + 1)
inline unsigned lag_live(long long n, int R, int E) {
  const long long taken = n / E + 1;
  return taken >= R ? (R == 32 ? ~0u : (1u << R) - 1u) : (1u << (int)taken) - 1u;
}

// the launch shape and the buffers
inline int lag_tiles(long long plane) { return (int)((plane + lag_limits::kTile - 1) / lag_limits::kTile); }
inline int lag_qtot(int nvars, int npairs, int R) { return nvars + R * npairs; }
inline size_t lag_origin_bytes(int nrep, int R, int nvars, long long nsites) { return (size_t)nrep * R * nvars * (size_t)nsites * sizeof(double); }
inline size_t lag_mask_bytes(int nrep, long long nsites, int persist_slot) { return persist_slot < 0 ? 0 : (size_t)nrep * (size_t)nsites * 2; }
// the stage buffer in 8-byte words: the partials [replica][z][qtot][tiles], the plane sums [replica][qtot][nz], the counters
// [replica][R] and the labels [replica][R]
inline size_t lag_stage_partials(int nrep, int nz, int qtot, int tiles) { return (size_t)nrep * nz * qtot * tiles; }
inline size_t lag_stage_planes(int nrep, int nz, int qtot) { return (size_t)nrep * qtot * nz; }
inline size_t lag_stage_words(int nrep, int nz, int qtot, int tiles, int R) {
  return lag_stage_partials(nrep, nz, qtot, tiles) + lag_stage_planes(nrep, nz, qtot) + 2 * (size_t)nrep * R;
}

}  // namespace

#ifndef BFLBM_LAG_HOST_ONLY

#include <memory>
#include <string>

struct bflbm_lag : bflbm_sample_store {      // d_rec [capacity][nrep][W] 8-byte words; d_stage: see lag_stage_words
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar
  int npairs = 0, R = 0, E = 1, W = 0, tiles = 0;
  LagPlan plan;                     // take and live are set per sample
  double* fields = nullptr;         // a batch: [nrep][nvars][nsites]
  double* origins = nullptr;        // [nrep][R][nvars][nsites]
  unsigned short* masks = nullptr;  // [nrep][nsites], only with persistence
  bflbm_lag() : bflbm_sample_store("lag trace", "bflbm_lag") {}
  ~bflbm_lag() override {
    if (fields || origins || masks) hipSetDevice(device);
    if (fields) hipFree(fields);
    if (origins) hipFree(origins);
    if (masks) hipFree(masks);
  }
  double* partials() const { return d_stage; }
  double* planes() const { return d_stage + lag_stage_partials(nrep, nz, plan.qtot, tiles); }
  unsigned long long* counters() const { return reinterpret_cast<unsigned long long*>(planes() + lag_stage_planes(nrep, nz, plan.qtot)); }
  long long* labels() const { return reinterpret_cast<long long*>(counters() + (size_t)nrep * R); }
  int record() override;
};

namespace {

struct LagSteps { long long s[lag_limits::kLabelChunk]; };

// the step counters of the replicas first .. first + n - 1 into the label of `slot`; one workgroup
__global__ void __launch_bounds__(64) k_lag_label(long long* __restrict__ labels, int R, int slot, int first, int n, LagSteps S) {
  const int i = (int)threadIdx.x;
  if (i < n) labels[(long long)(first + i) * R + slot] = S.s[i];
}

// The tree of profile_plane_z over the 256 per-thread sums of n quantities that every thread has written to
// buf[q * 256 + tid]: v[t] += v[t + w], w = 128 .. 1.  After one barrier wave k takes the quantities k, k + 4, ...: lane l
// forms (v[l] + v[l + 128]) + (v[l + 64] + v[l + 192]), which is what the levels 128 and 64 leave in v[l], then the lane
// shifts w = 32 .. 1; lane 0 stores quantity q at out[q * tiles + tile].  Every thread of the workgroup calls this
// together.  The caller alternates between two buffers, so a call needs no second barrier: whoever writes a buffer again
// has passed the barrier of the call between, which every reader of the buffer reached after its reads.
__device__ __forceinline__ void lag_tree(const double* __restrict__ buf, int n, double* __restrict__ out, int tiles, int tile) {
  const int lane = (int)threadIdx.x & 63;
  __syncthreads();
  for (int q = (int)threadIdx.x >> 6; q < n; q += 4) {
    const double* __restrict__ v = buf + q * 256 + lane;
    const double lo = v[0] + v[128], hi = v[64] + v[192];
    double s = lo + hi;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_down(s, w);
    if (lane == 0) out[(long long)q * tiles + tile] = s;
  }
}

// the 8 turns of a thread from one plane of one volume: p the plane's first site, s0 the thread's first turn
__device__ __forceinline__ void lag_load(const double* __restrict__ p, int s0, int odd, int plane, double (&x)[lag_limits::kPerThread]) {
  const bool al = fstat_aligned(p);
#pragma unroll
  for (int i = 0; i < lag_limits::kPerThread; i += 2) profile_two_turns(p, al, s0 + 256 * i, odd, 256, plane, x[i], x[i + 1]);
}

// grid (tiles of a plane, planes, replicas), 256 threads.  fields: the dense volumes, variable v of replica r at
// fields + r rep_stride + V.vol[v] nsites, [nz][plane]; origins [replica][R][NV][nsites]; masks [replica][nsites] or null;
// partial [replica][z][qtot][tiles]; counters [replica][R].  NV, the number of variables, is a template parameter: the
// current values are a register array of NV x 8 doubles.
// What the compiler reports (gfx950, -O3):
//   NV          1     2     3     4     5     6     7     8
//   VGPRs       82    108   125   149   157   181   189   213 
//   occupancy   4     4     4     3     3     2     2     2      waves per SIMD
// LDSByteSize 32832 (two buffers of 8 x 256 doubles for the tree and the 16 wave counters) and ScratchSize 0 in all eight instantiations
// (tests/test_lag_abi.py reads both from the listing).
template <int NV>
__global__ void __launch_bounds__(256) k_lag_products(const double* __restrict__ fields, long long rep_stride, long long nsites, int plane,
                                                      FstatVars V, LagPlan L, double* origins, unsigned short* masks,
                                                      double* __restrict__ partial, unsigned long long* __restrict__ counters) {
  using namespace lag_limits;
  __shared__ double sh[2][kMaxPairs * 256];               // the per-thread sums on their way into the tree, two buffers in turn
  __shared__ unsigned alive_sh[kMaxOrigins];
  const int tid = (int)threadIdx.x, odd = tid & 1;
  const int tile = (int)blockIdx.x, tiles = (int)gridDim.x, z = (int)blockIdx.y, rep = (int)blockIdx.z;
  const int s0 = tile * kTile + tid;
  const long long at = (long long)z * plane;
  if (tid < kMaxOrigins) alive_sh[tid] = 0u;               // the first tree's barriers come before any add

  double cur[NV][kPerThread];
#pragma unroll
  for (int v = 0; v < NV; ++v) lag_load(fields + (long long)rep * rep_stride + (long long)V.vol[v] * nsites + at, s0, odd, plane, cur[v]);

  double* __restrict__ out = partial + ((long long)rep * gridDim.y + z) * ((long long)L.qtot * tiles);
  int flip = 0;                                            // the buffer the next tree takes
#pragma unroll
  for (int v = 0; v < NV; ++v) {                           // now[v]: thread t adds its turns in order, then the tree
    double acc = 0.;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) acc += cur[v][i];
    sh[0][v * 256 + tid] = acc;
  }
  lag_tree(sh[0], NV, out, tiles, tile);
  flip ^= 1;

  double* const slots = origins + (long long)rep * L.R * NV * nsites + at;        // slot r, variable v: + (r NV + v) nsites
  if (L.take >= 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      double* __restrict__ o = slots + ((long long)L.take * NV + v) * nsites;
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) if (s0 + 256 * i < plane) o[s0 + 256 * i] = cur[v][i];
    }
  }

  // persistence: the masks of the thread's sites (0 past the plane: never counted) and the side of the current values
  unsigned m[kPerThread] = {};
  unsigned above = 0u;
  unsigned short* const mk = masks ? masks + (long long)rep * nsites + at : nullptr;
  if (mk) {
    double x[kPerThread];
    fstat_pick<NV, kPerThread>(cur, L.pslot, x);
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const bool in = s0 + 256 * i < plane;
      m[i] = in ? (unsigned)mk[s0 + 256 * i] : 0u;
      if (in && L.take >= 0) m[i] |= 1u << L.take;
      above |= (x[i] >= L.level ? 1u : 0u) << i;           // a NaN: false
    }
  }

#pragma unroll 1
  for (int r = 0; r < L.R; ++r) {
    if (!((L.live >> r) & 1u)) continue;
    const bool fresh = r == L.take;                        // its origin is the current values: the registers
    const double* const org = slots + (long long)r * NV * nsites;
#pragma unroll 1
    for (int p = 0; p < L.npairs; ++p) {                   // one pair at a time: 8 doubles of the origin in flight per thread
      double a[kPerThread], b[kPerThread];
      fstat_pick<NV, kPerThread>(cur, L.pa[p], a);
      if (fresh) fstat_pick<NV, kPerThread>(cur, L.pb[p], b);
      else lag_load(org + (long long)L.pb[p] * nsites, s0, odd, plane, b);
      double acc = 0.;
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) { const double q = a[i] * b[i]; acc += q; }   // the product first, then the sum
      sh[flip][p * 256 + tid] = acc;
    }
    lag_tree(sh[flip], L.npairs, out + (long long)(NV + r * L.npairs) * tiles, tiles, tile);
    flip ^= 1;
    if (mk) {
      if (!fresh) {                                        // a fresh origin is on its own side everywhere
        double b[kPerThread];
        lag_load(org + (long long)L.pslot * nsites, s0, odd, plane, b);
#pragma unroll
        for (int i = 0; i < kPerThread; ++i) {
          const bool same = (b[i] >= L.level) == (((above >> i) & 1u) != 0u);
          if (!same) m[i] &= ~(1u << r);
        }
      }
      unsigned n = 0u;                                     // wave-uniform
#pragma unroll
      for (int i = 0; i < kPerThread; ++i) n += (unsigned)__popcll(__ballot((m[i] >> r) & 1u));
      if ((tid & 63) == 0 && n) atomicAdd(&alive_sh[r], n);
    }
  }

  if (mk) {
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) if (s0 + 256 * i < plane) mk[s0 + 256 * i] = (unsigned short)m[i];
    __syncthreads();
    if (tid < L.R) {
      const unsigned n = alive_sh[tid];
      if (n) atomicAdd(&counters[(long long)rep * L.R + tid], (unsigned long long)n);
    }
  }
}

// grid (ceil(nz qtot / 256), replicas): thread (z, q) adds, starting from +0.0, the tiles of plane z in tile order into
// planes [replica][qtot][nz].  The sums of a slot that is not live are skipped: nothing wrote their partials.
__global__ void __launch_bounds__(256) k_lag_planes(const double* __restrict__ partial, double* __restrict__ planes, int nz, int tiles, int nvars,
                                                    LagPlan L) {
  const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= nz * L.qtot) return;
  const int z = g / L.qtot, q = g - z * L.qtot;
  if (q >= nvars && !((L.live >> ((q - nvars) / L.npairs)) & 1u)) return;
  const double* __restrict__ p = partial + (((long long)blockIdx.y * nz + z) * L.qtot + q) * tiles;
  double s = 0.;
  for (int t = 0; t < tiles; ++t) s += p[t];
  planes[((long long)blockIdx.y * L.qtot + q) * nz + z] = s;
}

// grid (replicas), 256 threads: thread w < W writes word w of the replica's sample: the planes z = 0 .. nz-1 in sequence
// from +0.0 (now, corr), the label, the counter (which goes back to zero).  An empty slot: -1, -1, NaN.
__global__ void __launch_bounds__(256) k_lag_finish(const double* __restrict__ planes, unsigned long long* __restrict__ counters,
                                                    const long long* __restrict__ labels, double* __restrict__ out, int nz, int nvars, LagPlan L) {
  const int w = (int)threadIdx.x, per = 2 + L.npairs, W = nvars + L.R * per;
  if (w >= W) return;
  const long long rep = blockIdx.x;
  double* __restrict__ word = out + rep * W + w;
  int q = w;                                               // the sum this word holds, or -1
  if (w >= nvars) {
    const int r = (w - nvars) / per, j = (w - nvars) - r * per;
    const bool live = (L.live >> r) & 1u;
    if (j == 0) {
      *reinterpret_cast<long long*>(word) = live ? labels[rep * L.R + r] : -1ll;
      return;
    }
    if (j == 1) {
      unsigned long long* __restrict__ c = counters + rep * L.R + r;
      *reinterpret_cast<long long*>(word) = (live && L.pslot >= 0) ? (long long)*c : -1ll;
      *c = 0ull;
      return;
    }
    if (!live) { *word = __longlong_as_double(0x7ff8000000000000ll); return; }
    q = nvars + r * L.npairs + (j - 2);
  }
  const double* __restrict__ p = planes + (rep * L.qtot + q) * nz;
  double s = 0.;
  for (int z = 0; z < nz; ++z) s += p[z];
  *word = s;
}

int lag_create(bflbm_ctx* c, bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
               int norigins, int origin_stride, int persist_slot, double persist_level, int every, long long capacity, bflbm_lag** out) {
  using namespace lag_limits;
  const char* call = b ? "bflbm_batch_lag_create" : "bflbm_lag_create";
  if (lag_refuse_args(call, source, nvars, vars, npairs, pair_a, pair_b, norigins, origin_stride, persist_slot, persist_level)) return 1;
  if (store_refuse_cadence(call, every, capacity)) return 1;
  const int nrep = b ? (int)b->ctx.size() : 1;
  const int W = lag_words(nvars, npairs, norigins);
  const size_t per = (size_t)nrep * W;
  const std::string shape = " x " + std::to_string(W) + " words";
  if (store_refuse_capacity(call, capacity, per, nrep, shape.c_str())) return 1;
  if (store_refuse_owner(c, call, "bflbm_batch_lag_create", "lag trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if (G.nz > kMaxPlanes) return fail("%s: nz = %d exceeds the %d planes of one launch", call, G.nz, kMaxPlanes);

  std::unique_ptr<bflbm_lag> t(new bflbm_lag());
  recorder_bind(t.get(), c, b, every);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  t->npairs = npairs; t->R = norigins; t->E = origin_stride; t->W = W;
  t->tiles = lag_tiles((long long)G.nx * G.ny);
  LagPlan& L = t->plan;
  L.R = norigins; L.npairs = npairs;
  for (int p = 0; p < kMaxPairs; ++p) { L.pa[p] = p < npairs ? pair_a[p] : 0; L.pb[p] = p < npairs ? pair_b[p] : 0; }
  L.take = -1; L.live = 0u;
  L.pslot = persist_slot; L.level = persist_slot >= 0 ? persist_level : 0.;
  L.qtot = lag_qtot(nvars, npairs, norigins);

  const size_t ob = lag_origin_bytes(nrep, norigins, nvars, t->nsites), mb = lag_mask_bytes(nrep, t->nsites, persist_slot);
  const size_t fb = b ? (size_t)nrep * nvars * (size_t)t->nsites * sizeof(double) : 0;
  const size_t stage = lag_stage_words(nrep, G.nz, L.qtot, t->tiles, norigins);
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->origins, ob);
  if (e == hipSuccess && mb) e = hipMalloc((void**)&t->masks, mb);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu bytes, origins %zu, masks %zu; then stage %zu + records %zu x %lld): %s", call, fb, ob, mb,
                stage * sizeof(double), per * sizeof(double), capacity, hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, stage, shape.c_str())) return 1;
  // The counters and the labels are in the store's stage buffer, so their first values come after the owner's list took
  // the trace: a failure detaches again (store_destroy), as the histogram trace's zeroing does.
  bflbm_lag* g = t.release();
  const hipStream_t stream = recorder_stream(g);
  e = hipMemsetAsync(g->counters(), 0, (size_t)nrep * norigins * sizeof(long long), stream);
  if (e == hipSuccess) e = hipMemsetAsync(g->labels(), 0xff, (size_t)nrep * norigins * sizeof(long long), stream);
  if (e == hipSuccess && mb) e = hipMemsetAsync(g->masks, 0, mb, stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(g);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = g;
  return 0;
}

}  // namespace

// enqueue the observation, the label of a new origin, the summing launch and the two finishing launches of the resident
// state into slot n; no host synchronisation
int bflbm_lag::record() {
  using namespace lag_limits;
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "lag trace sample", &dense, &rep_stride)) return 1;
  plan.take = lag_take(n, R, E);
  plan.live = lag_live(n, R, E);
  if (plan.take >= 0) {
    for (int first = 0; first < nrep; first += kLabelChunk) {
      LagSteps S;
      const int cnt = std::min(kLabelChunk, nrep - first);
      for (int i = 0; i < kLabelChunk; ++i) S.s[i] = i < cnt ? (batch ? batch->ctx[first + i]->steps : ctx->steps) : 0;
      hipLaunchKernelGGL(k_lag_label, dim3(1), dim3(64), 0, stream, labels(), R, plan.take, first, cnt, S);
    }
    HIP_TRY(hipGetLastError());
  }
  const int plane = nx * ny;
  const dim3 grid((unsigned)tiles, (unsigned)nz, (unsigned)nrep);
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_lag_products<decltype(nv)::value>), grid, dim3(256), 0, stream, dense, rep_stride, nsites, plane, fs.vol, plan,
                           origins, masks, partials(), counters());
      })) return fail("lag trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_lag_planes, dim3((unsigned)((nz * plan.qtot + 255) / 256), (unsigned)nrep), dim3(256), 0, stream,
                     partials(), planes(), nz, tiles, fs.nvars, plan);
  hipLaunchKernelGGL(k_lag_finish, dim3((unsigned)nrep), dim3(256), 0, stream, planes(), counters(), labels(), store_slot(this), nz, fs.nvars, plan);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_lag_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b, int norigins,
                     int origin_stride, int persist_slot, double persist_level, int every, long long capacity, bflbm_lag** out) {
  if (!c || !vars || !pair_a || !pair_b || !out) return fail("bflbm_lag_create: null argument");
  return lag_create(c, nullptr, source, nvars, vars, npairs, pair_a, pair_b, norigins, origin_stride, persist_slot, persist_level, every, capacity, out);
}
int bflbm_batch_lag_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b, int norigins,
                           int origin_stride, int persist_slot, double persist_level, int every, long long capacity, bflbm_lag** out) {
  if (!b || !vars || !pair_a || !pair_b || !out) return fail("bflbm_batch_lag_create: null argument");
  return lag_create(nullptr, b, source, nvars, vars, npairs, pair_a, pair_b, norigins, origin_stride, persist_slot, persist_level, every, capacity, out);
}

int bflbm_lag_destroy(bflbm_lag* t) { return store_destroy(t); }
int bflbm_lag_sample(bflbm_lag* t) { return store_sample(t, "bflbm_lag"); }
// also empties the slots: n restarts, so the schedule does, and the labels read -1 until a slot is taken again
int bflbm_lag_reset(bflbm_lag* t) {
  if (store_reset(t, "bflbm_lag")) return 1;
  t->plan.take = -1; t->plan.live = 0u;
  if (recorder_attached(t)) {
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipMemsetAsync(t->labels(), 0xff, (size_t)t->nrep * t->R * sizeof(long long), recorder_stream(t)));
  }
  return 0;
}
int bflbm_lag_count(const bflbm_lag* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_lag", nsamples, nreplicas); }
int bflbm_lag_read(bflbm_lag* t, long long first, long long count, double* words, long long* steps) {
  return store_read(t, "bflbm_lag", first, count, words, steps);   // 8-byte words, copied bit for bit
}

int bflbm_lag_geometry(const bflbm_lag* t, int* nvars, int* npairs, int* norigins, int* origin_stride, int* words, int* tile_sites,
                       int* tiles_per_plane, long long* origin_bytes, long long* mask_bytes) {
  if (!t) return fail("bflbm_lag_geometry: null argument");
  if (nvars) *nvars = t->fs.nvars;
  if (npairs) *npairs = t->npairs;
  if (norigins) *norigins = t->R;
  if (origin_stride) *origin_stride = t->E;
  if (words) *words = t->W;
  if (tile_sites) *tile_sites = lag_limits::kTile;
  if (tiles_per_plane) *tiles_per_plane = t->tiles;
  if (origin_bytes) *origin_bytes = (long long)lag_origin_bytes(t->nrep, t->R, t->fs.nvars, t->nsites);
  if (mask_bytes) *mask_bytes = (long long)lag_mask_bytes(t->nrep, t->nsites, t->plan.pslot);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_LAG_HOST_ONLY

#endif  // BFLBM_LAG_H_
