// bflbm_profile.h -- profile traces: the sums of chosen hydrovs or hydrovsbar components, and of chosen products of
// them, over every lattice plane normal to one axis, recorded on the device as a time series for a lone single-slab
// context, every replica of a batch or a ring of z-slabs (include/bflbm.h, "Profile traces": the definition and the
// order of every sum are stated there and only there).  rho(z) and phi(z) across a flat interface and the
// normal-minus-tangential pressure -(af_n ag_n - af_t ag_t) / alpha0, whose integral is the mechanical surface tension,
// are plane means; without this a user downloads 22 fields per replica and sample and averages them on the host.
// A sample is, on the owner's stream(s) and without a host synchronisation,
//   the accumulators' observation   batch_observe_launch into the trace's [B][nsel][n] / observe_launch into the
//                                   scratch state buffer of the context (of every slab of a ring),
//   k_profile_planes<NV>            stage 1, grid (work items of a plane, planes, replicas): a site's variables are
//                                   loaded once, the products are formed in registers, one partial per (q, work item):
//                                   [replica][z][q][W], W the tiles of a plane (axis z), ny (axis y) or nx (axis x),
//   k_profile_finish                stage 2: the tiles of a plane in order (axis z) or the planes in sequence (axes x, y),
//                                   straight into the slot.
// A ring: stage 1 on every slab's stream over its own planes into [nzl][q][W]; slab 0 takes the other slabs' blocks
// to their planes' place in its stage buffer (the ring gather of bflbm_recorder.h), the unchanged stage 2 runs on
// slab 0.  No atomics, no scratch.  Not built on purpose: reading the populations in stage 1 to skip the dense
// intermediate (hydrovs needs the gradient stencil the observation already has), fusing the sums into the observation
// kernels (it would give every observer a second form), the kinetic rho u u part of the tensor as a built-in (the
// caller's own pairs give it).
// The lifecycle and the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by
// bflbm.hip after bflbm_fstat.h (needs bflbm_ctx, bflbm_batch, bflbm_ring, FieldSelection, FstatVars, FstatPairs,
// fields_observe, field_dispatch_nv, ring_prepare_ref, fstat_pick, fstat_aligned).
#ifndef BFLBM_PROFILE_H_
#define BFLBM_PROFILE_H_

#include <memory>
#include <string>
#include <vector>

namespace profile_limits {
constexpr int kMaxVars = fstat_limits::kMaxVars, kMaxPairs = fstat_limits::kMaxPairs;
constexpr int kTile = 2048;          // axis z: sites per workgroup, 8 per thread, as the mode trace.  An untimed heuristic.
constexpr int kPerThread = kTile / 256;
constexpr int kLanes = 64;           // axis y: the lanes that stride a row (one wave per row)
constexpr int kChunk = 64;           // axis x: rows per chunk of a column
}

struct bflbm_profile : bflbm_sample_store {   // d_rec [capacity][nrep][nq][na], d_stage [nrep][nz][nq][W]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar
  int axis = 2, na = 0;             // the axis and its extent
  int nq = 0;                       // nq = nvars + npairs
  int W = 0;                        // partials per (q, plane) that stage 1 leaves
  FstatPairs pairs;
  double* fields = nullptr;         // a batch: [nrep][nvars][nsites]
  RingGather gather;                // a ring: slab k's block is [nzl][nq][W] (slab 0 writes d_stage itself)
  bflbm_profile() : bflbm_sample_store("profile trace", "bflbm_profile") {}
  ~bflbm_profile() override {
    if (fields) { hipSetDevice(device); hipFree(fields); }
  }
  int record() override;
  int record_ring();
  int stage1(const double* dense, long long rep_stride, long long comp_stride, double* partial, int planes, int reps, hipStream_t stream) const;
};

namespace {

// one site (W = 1) into the accumulators: the variables, then every pair, the product formed first and then added.  The
// loop over the pairs is unrolled to its limit, so every accumulator has a compile-time index and stays in a register;
// the slots are uniform and picked by selects.
template <int NV, int W>
__device__ __forceinline__ void profile_add(double (&acc)[NV + profile_limits::kMaxPairs][W], const double (&x)[NV][W], const FstatPairs& P) {
#pragma unroll
  for (int v = 0; v < NV; ++v) {
#pragma unroll
    for (int i = 0; i < W; ++i) acc[v][i] += x[v][i];
  }
#pragma unroll
  for (int p = 0; p < profile_limits::kMaxPairs; ++p) {
    if (p < P.n) {
      double a[W], b[W];
      fstat_pick<NV, W>(x, P.a[p], a);
      fstat_pick<NV, W>(x, P.b[p], b);
#pragma unroll
      for (int i = 0; i < W; ++i) { const double q = a[i] * b[i]; acc[NV + p][i] += q; }
    }
  }
}

// The values a lane adds in two consecutive turns: entries s and s + stride of p, 0 past `limit`.  The lanes 2 k and
// 2 k + 1 sit on neighbouring entries in both turns.  Where p is 16-byte aligned and both turns lie inside, the even
// lane loads the pair of the first turn and the odd lane the pair of the second with one 16-byte access each, and the
// two swap halves; otherwise two 8-byte loads.  `odd`: the lane's parity, which is the parity of s.  Every lane of the
// wave calls this together.
__device__ __forceinline__ void profile_two_turns(const double* __restrict__ p, bool aligned, int s, int odd, int stride, int limit,
                                                  double& first, double& second) {
  const int se = s - odd;
  const bool wide = aligned && se + stride + 1 < limit;
  double2 m = make_double2(0., 0.);
  if (wide) m = *reinterpret_cast<const double2*>(p + (odd ? se + stride : se));
  const double got = __shfl_xor(odd ? m.x : m.y, 1);
  if (wide) { first = odd ? got : m.x; second = odd ? m.y : got; }
  else { first = s < limit ? p[s] : 0.; second = s + stride < limit ? p[s + stride] : 0.; }
}

// axis z, grid.x = tiles: thread t adds the sites t, t + 256, ... of its tile, the tree of block_reduce over the 256 sums
// (levels 128 and 64 through LDS, the rest by lane shifts in wave 0).  vol[v]: variable v on this plane; out: [nq][tiles].
template <int NV>
__device__ __forceinline__ void profile_plane_z(const double* (&vol)[NV], int plane, const FstatPairs& P, int nq,
                                                double* __restrict__ out, double* __restrict__ sh) {
  using namespace profile_limits;
  constexpr int NQ = NV + kMaxPairs;
  const int tid = (int)threadIdx.x, odd = tid & 1;
  const int s0 = (int)blockIdx.x * kTile + tid;
  double acc[NQ][1];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q][0] = 0.;
  bool al[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) al[v] = fstat_aligned(vol[v]);
#pragma unroll
  for (int i = 0; i < kPerThread; i += 2) {
    double x0[NV][1], x1[NV][1];
#pragma unroll
    for (int v = 0; v < NV; ++v) profile_two_turns(vol[v], al[v], s0 + 256 * i, odd, 256, plane, x0[v][0], x1[v][0]);
    profile_add<NV, 1>(acc, x0, P);
    profile_add<NV, 1>(acc, x1, P);
  }
  double* __restrict__ xa = sh;                          // [NQ][128]: waves 2, 3 to waves 0, 1
  double* __restrict__ xb = sh + NQ * 128;               // [NQ][64]: wave 1 to wave 0
  if (tid >= 128) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) if (q < nq) xa[q * 128 + tid - 128] = acc[q][0];
  }
  __syncthreads();
  if (tid < 128) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) if (q < nq) acc[q][0] += xa[q * 128 + tid];
    if (tid >= 64) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) if (q < nq) xb[q * 64 + tid - 64] = acc[q][0];
    }
  }
  __syncthreads();
  if (tid < 64) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nq) {
        double v = acc[q][0] + xb[q * 64 + tid];
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) v += __shfl_down(v, w);
        if (tid == 0) out[(long long)q * gridDim.x + blockIdx.x] = v;
      }
    }
  }
}

// axis y, grid.x = ceil(ny / 4): one wave per row; lane l adds x = l, l + 64, ..., then the tree w = 32 .. 1 by lane
// shifts.  out: [nq][ny].
template <int NV>
__device__ __forceinline__ void profile_plane_y(const double* (&vol)[NV], int nx, int ny, const FstatPairs& P, int nq,
                                                double* __restrict__ out) {
  using namespace profile_limits;
  constexpr int NQ = NV + kMaxPairs;
  const int lane = (int)threadIdx.x & 63, odd = lane & 1;
  const int y = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (y >= ny) return;                                   // the whole wave
  double acc[NQ][1];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q][0] = 0.;
  const double* row[NV];
  bool al[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) { row[v] = vol[v] + (long long)y * nx; al[v] = fstat_aligned(row[v]); }
  const int turns = (nx + kLanes - 1) / kLanes;
  int k = 0;
  for (; k + 1 < turns; k += 2) {
    double x0[NV][1], x1[NV][1];
#pragma unroll
    for (int v = 0; v < NV; ++v) profile_two_turns(row[v], al[v], lane + kLanes * k, odd, kLanes, nx, x0[v][0], x1[v][0]);
    profile_add<NV, 1>(acc, x0, P);
    profile_add<NV, 1>(acc, x1, P);
  }
  if (k < turns) {
    const int x = lane + kLanes * k;
    double x0[NV][1];
#pragma unroll
    for (int v = 0; v < NV; ++v) x0[v][0] = x < nx ? row[v][x] : 0.;
    profile_add<NV, 1>(acc, x0, P);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q < nq) {
      double v = acc[q][0];
#pragma unroll
      for (int w = 32; w > 0; w >>= 1) v += __shfl_down(v, w);
      if (lane == 0) out[(long long)q * ny + y] = v;
    }
  }
}

// axis x, grid.x = ceil(nx / 64): lane l owns column x = 64 blockIdx.x + l (8-byte loads, a wave reads 512 contiguous
// bytes of a row); the four waves take the chunks c = w, w + 4, ... of 64 rows, each added sequentially in y from 0;
// per round of four chunks the waves 1 .. 3 hand theirs to wave 0 through LDS, which adds the chunks in order.  A chunk
// past the plane hands over +0.0, which changes no sum that started from +0.0.  out: [nq][nx].
template <int NV>
__device__ __forceinline__ void profile_plane_x(const double* (&vol)[NV], int nx, int ny, const FstatPairs& P, int nq,
                                                double* __restrict__ out, double* __restrict__ sh) {
  using namespace profile_limits;
  constexpr int NQ = NV + kMaxPairs;
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  const int x = (int)blockIdx.x * 64 + lane;
  const int nchunks = (ny + kChunk - 1) / kChunk;
  double total[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) total[q] = 0.;
  for (int c0 = 0; c0 < nchunks; c0 += 4) {
    double acc[NQ][1];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q][0] = 0.;
    const int c = c0 + w;
    if (c < nchunks && x < nx) {
      const int y1 = min(ny, (c + 1) * kChunk);
#pragma unroll 4
      for (int y = c * kChunk; y < y1; ++y) {
        double x0[NV][1];
#pragma unroll
        for (int v = 0; v < NV; ++v) x0[v][0] = vol[v][(long long)y * nx + x];
        profile_add<NV, 1>(acc, x0, P);
      }
    }
    if (w > 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) if (q < nq) sh[((w - 1) * NQ + q) * 64 + lane] = acc[q][0];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
          total[q] += acc[q][0];
#pragma unroll
          for (int u = 0; u < 3; ++u) total[q] += sh[(u * NQ + q) * 64 + lane];
        }
      }
    }
    __syncthreads();
  }
  if (w == 0 && x < nx) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) if (q < nq) out[(long long)q * nx + x] = total[q];
  }
}

// Stage 1, grid (work items of a plane, planes, replicas), 256 threads.  fields: the dense volumes, variable v of
// replica r at fields + r rep_stride + V.vol[v] comp_stride, [planes][ny][nx]; partial: [replica][plane][nq][W].  NV, the
// number of variables, is a template parameter: the site values and the accumulators are register arrays of that size.
template <int NV>
__global__ void __launch_bounds__(256) k_profile_planes(const double* __restrict__ fields, long long rep_stride, long long comp_stride,
                                                        double* __restrict__ partial, int nx, int ny, int axis, int W,
                                                        FstatVars V, FstatPairs P) {
  __shared__ double sh[(NV + profile_limits::kMaxPairs) * 192];
  const int plane = nx * ny, nq = NV + P.n;
  const double* vol[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v)
    vol[v] = fields + (long long)blockIdx.z * rep_stride + (long long)V.vol[v] * comp_stride + (long long)blockIdx.y * plane;
  double* __restrict__ out = partial + ((long long)blockIdx.z * gridDim.y + blockIdx.y) * ((long long)nq * W);
  if (axis == 2) profile_plane_z<NV>(vol, plane, P, nq, out, sh);
  else if (axis == 1) profile_plane_y<NV>(vol, nx, ny, P, nq, out);
  else profile_plane_x<NV>(vol, nx, ny, P, nq, out, sh);
}

// Stage 2, grid (ceil(nq na / 256), replicas): thread (q, i) adds, starting from 0, the W tiles of plane i in tile
// order (axis z) or entry i of the planes z = 0 .. nz-1 in sequence (axes x, y).  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_profile_finish(const double* __restrict__ partial, double* __restrict__ out,
                                                        int axis, int nz, int nq, int W, int na) {
  const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (g >= nq * na) return;
  const int q = g / na, i = g - q * na;
  const double* __restrict__ mine = partial + (long long)blockIdx.y * nz * nq * W;
  double s = 0.;
  if (axis == 2) {
    const double* __restrict__ p = mine + ((long long)i * nq + q) * W;
    for (int t = 0; t < W; ++t) s += p[t];
  } else {
    const double* __restrict__ p = mine + (long long)q * W + i;
    for (int z = 0; z < nz; ++z) s += p[(long long)z * nq * W];
  }
  out[((long long)blockIdx.y * nq + q) * na + i] = s;
}

int profile_create(bflbm_ctx* c, bflbm_batch* b, bflbm_ring* g, int source, int axis, int nvars, const int* vars, int npairs,
                   const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_profile** out) {
  using namespace profile_limits;
  const char* call = b ? "bflbm_batch_profile_create" : (g ? "bflbm_ring_profile_create" : "bflbm_profile_create");
  if (field_refuse_args(call, source, 1, nvars, vars, npairs, pair_a, pair_b)) return 1;
  if (axis < 0 || axis > 2) return fail("%s: axis must be 0 (x), 1 (y) or 2 (z) (got %d)", call, axis);
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_profile_create", "profile trace")) return 1;
  if (recorder_refuse_open(c, b, g, call)) return 1;
  const Geo& G = c ? c->G : (b ? b->G : g->ctx[0]->G);
  if (G.nz > 65535) return fail("%s: nz = %d exceeds the 65535 planes of one launch", call, G.nz);

  std::unique_ptr<bflbm_profile> t(new bflbm_profile());
  recorder_bind(t.get(), c, b, every, g);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->axis = axis; t->nq = nvars + npairs;
  t->na = axis == 0 ? G.nx : (axis == 1 ? G.ny : G.nz);
  t->W = axis == 2 ? (G.nx * G.ny + kTile - 1) / kTile : t->na;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  t->pairs = field_pairs(npairs, pair_a, pair_b);

  const size_t per = (size_t)t->nrep * t->nq * t->na;
  const size_t plane_doubles = (size_t)t->nq * t->W, stage = (size_t)t->nrep * G.nz * plane_doubles;
  const std::string shape = " x " + std::to_string(t->nq) + " sums x " + std::to_string(t->na) + " planes";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the fields of a batch
  const size_t fb = b ? (size_t)t->nrep * nvars * (size_t)t->nsites * sizeof(double) : 0;
  const size_t plane_bytes = plane_doubles * sizeof(double);
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e == hipSuccess && g) e = gather_create(t->gather, g, [&](int k) { return (size_t)g->ctx[k]->nzl * plane_bytes; },
                                              [&](int k) { return (size_t)g->ctx[k]->dom.z0 * plane_bytes; });
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu bytes, slab partials %zu per plane; then records %zu x %lld + plane partials %zu): %s",
                call, fb, g ? plane_bytes : (size_t)0, per * sizeof(double), capacity, stage * sizeof(double), hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, stage, shape.c_str(), g)) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// the stage 1 launch over `planes` planes of `reps` replicas on `stream`
int bflbm_profile::stage1(const double* dense, long long rep_stride, long long comp_stride, double* partial, int planes, int reps,
                          hipStream_t stream) const {
  using namespace profile_limits;
  const unsigned items = axis == 2 ? (unsigned)W : (axis == 1 ? (unsigned)((ny + 3) / 4) : (unsigned)((nx + 63) / 64));
  const dim3 grid(items, (unsigned)planes, (unsigned)reps);
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_profile_planes<decltype(nv)::value>), grid, dim3(256), 0, stream, dense, rep_stride, comp_stride, partial, nx, ny, axis, W, fs.vol, pairs);
      })) return fail("profile trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  return 0;
}

// enqueue the observation and the two stages of the resident state into slot n; no host synchronisation
int bflbm_profile::record() {
  if (ring) return record_ring();
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "profile trace sample", &dense, &rep_stride)) return 1;
  if (stage1(dense, rep_stride, nsites, d_stage, nz, nrep, stream)) return 1;
  hipLaunchKernelGGL(k_profile_finish, dim3((unsigned)((nq * na + 255) / 256), (unsigned)nrep), dim3(256), 0, stream,
                     d_stage, store_slot(this), axis, nz, nq, W, na);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

int bflbm_profile::record_ring() {
  if (store_begin(this)) return 1;
  if (fs.source != 1 && ring_prepare_ref(ring)) return 1;  // the global centre of mass: the slabs' own prepare_ref is then a no-op
  const int n = (int)ring->ctx.size();
  const long long plane = (long long)nx * ny;
  for (int k = 0; k < n; ++k) {
    bflbm_ctx* c = ring->ctx[k];
    const double* dense;
    if (fields_observe_slab(c, fs, "profile trace sample", &dense)) return 1;         // selects the slab's device
    if (gather_hold(gather, k, c->stream)) return 1;
    if (stage1(dense, 0, (long long)c->nzl * plane, gather_target(gather, k, d_stage), c->nzl, 1, c->stream)) return 1;
    if (gather_ready(gather, k, c->stream)) return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const hipStream_t s0 = ring->ctx[0]->stream;
  if (gather_take(gather, d_stage, s0)) return 1;
  hipLaunchKernelGGL(k_profile_finish, dim3((unsigned)((nq * na + 255) / 256), 1), dim3(256), 0, s0,
                     d_stage, store_slot(this), axis, nz, nq, W, na);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_profile_create(bflbm_ctx* c, int source, int axis, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                         int every, long long capacity, bflbm_profile** out) {
  if (!c || !vars || !out) return fail("bflbm_profile_create: null argument");
  return profile_create(c, nullptr, nullptr, source, axis, nvars, vars, npairs, pair_a, pair_b, every, capacity, out);
}
int bflbm_batch_profile_create(bflbm_batch* b, int source, int axis, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                               int every, long long capacity, bflbm_profile** out) {
  if (!b || !vars || !out) return fail("bflbm_batch_profile_create: null argument");
  return profile_create(nullptr, b, nullptr, source, axis, nvars, vars, npairs, pair_a, pair_b, every, capacity, out);
}
int bflbm_ring_profile_create(bflbm_ring* r, int source, int axis, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                              int every, long long capacity, bflbm_profile** out) {
  if (!r || !vars || !out) return fail("bflbm_ring_profile_create: null argument");
  if (r->ctx.size() == 1)                                  // the whole box: the lone recorder of ctx[0], served by its steps
    return profile_create(r->ctx[0], nullptr, nullptr, source, axis, nvars, vars, npairs, pair_a, pair_b, every, capacity, out);
  return profile_create(nullptr, nullptr, r, source, axis, nvars, vars, npairs, pair_a, pair_b, every, capacity, out);
}

int bflbm_profile_destroy(bflbm_profile* t) { return store_destroy(t); }
int bflbm_profile_sample(bflbm_profile* t) { return store_sample(t, "bflbm_profile"); }
int bflbm_profile_reset(bflbm_profile* t) { return store_reset(t, "bflbm_profile"); }
int bflbm_profile_count(const bflbm_profile* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_profile", nsamples, nreplicas); }
int bflbm_profile_read(bflbm_profile* t, long long first, long long count, double* sums, long long* steps) {
  return store_read(t, "bflbm_profile", first, count, sums, steps);
}

int bflbm_profile_geometry(const bflbm_profile* t, int* nsums, int* n_axis, int* tile_sites, int* tiles_per_plane) {
  using namespace profile_limits;
  if (!t) return fail("bflbm_profile_geometry: null argument");
  if (nsums) *nsums = t->nq;
  if (n_axis) *n_axis = t->na;
  if (tile_sites) *tile_sites = t->axis == 2 ? kTile : (t->axis == 1 ? kLanes : kChunk);
  if (tiles_per_plane) *tiles_per_plane = t->W;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_PROFILE_H_
