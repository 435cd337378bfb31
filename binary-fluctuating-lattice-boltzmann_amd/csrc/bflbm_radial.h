// bflbm_radial.h -- radial traces: the sums of chosen hydrovs or hydrovsbar components, of chosen products of them and of
// chosen projections onto the outward radial unit vector, over the shells of width delta about a droplet's centre,
// recorded on the device as a time series for a lone single-slab context or every replica of a batch (include/bflbm.h,
// "Radial traces": the definition and the order of every sum are stated there and only there).  The pressure inside and
// outside a droplet, the Shan-Chen force integrated from the edge to the centre and rho(r) for a radius are shell means;
// without this a user downloads 22 fields per replica and sample and bins them on the host.  It is the profile trace
// turned from planes into shells; new is that the bin of a site is data-dependent (the centre moves), so the bins cannot
// be owned by threads that also own the sites.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   batch_observe_launch into the trace's [B][nsel][n] / observe_launch into the scratch
//                                   state buffer of the context, as the profile trace takes it,
//   with a null centre              trace_moments_launch of bflbm_trace.h into the trace's own [nrep][12], as
//                                   bflbm_shape.h does: the centre is Trace.com() of the state bit for bit,
//   k_radial_shells<NV>             grid (planes, replicas): the workgroup walks the tiles of 256 sites of its plane in
//                                   order.  Per tile every thread loads its site's variables once, forms the image
//                                   vector, r, the shell and the projections and stages variables, projections and shell
//                                   in LDS; the tile's lowest and highest shell come from an integer reduction (lane
//                                   exchanges, then four values through LDS); every thread owns the items
//                                   (shell, term) = divmod(t + 256 j, 1 + Q), and for those inside the tile's shell range
//                                   walks the tile's sites in order (the shell a broadcast LDS read), adds the members'
//                                   terms from +0.0 (products formed on the fly from the staged rows) and then adds
//                                   the tile's partial to its per-plane accumulator in a register.  One
//                                   [1 + Q][nbins] block per (replica, plane) leaves the kernel,
//   k_radial_finish                 one thread per (replica, term, shell) adds the planes in sequence straight into the
//                                   slot, three more write the centre.
// No atomics, no scratch.  The loads are 8 bytes per lane (a wave reads 512 contiguous bytes of a variable): a lane owns
// one site of a tile, so a 16-byte load would need the lane-pair exchange of bflbm_profile.h over two tiles at once.
// The lifecycle and the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by
// bflbm.hip after bflbm_profile.h (needs bflbm_ctx, bflbm_batch, FieldSelection, FstatVars, fields_observe,
// field_dispatch_nv, fstat_pick, trace_moments_launch, kNTrace, shape_centre).
#ifndef BFLBM_RADIAL_H_
#define BFLBM_RADIAL_H_

#include <memory>
#include <string>

namespace radial_limits {
constexpr int kMaxVars = fstat_limits::kMaxVars, kMaxPairs = fstat_limits::kMaxPairs, kMaxRad = 4, kMaxBins = 128;
constexpr int kTile = 256;                                       // sites of a tile = threads of a workgroup.  An untimed heuristic.
constexpr int kMaxTerms = 1 + kMaxVars + kMaxPairs + kMaxRad;    // the count term first
constexpr int kMaxItems = (kMaxTerms * kMaxBins + 255) / 256;    // (shell, term) items a thread can own
}

// A term is (row a) * (row b) of the staged rows: 0 .. NV-1 the variables, NV + k the projection of radial term k, -1 the
// constant 1.0 (x * 1.0 == x bit for bit).  The count is (-1, -1), a variable (v, -1), a pair (a, b), a radial term
// (NV + k, -1) or (w, NV + k).  By value.
struct RadialTerms { int n; signed char a[radial_limits::kMaxTerms]; signed char b[radial_limits::kMaxTerms]; };
struct RadialRads { int n; int v[radial_limits::kMaxRad][3]; };

// d_rec [capacity][nrep][3 + (1 + Q) nbins]; d_stage = planes [nrep][nz][(1 + Q) nbins] | moments [nrep][12] | block sums
// [nrep][nz][plane blocks][12] (the last two: null centre) | fields [nrep][nvars][nsites] (a batch)
struct bflbm_radial : bflbm_sample_store {
  Geo G;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar
  int nq = 0, nbins = 0;            // nq = nvars + npairs + nrad
  int W = 0;                        // tiles per plane
  RadialTerms terms;
  RadialRads rads;
  bool com = false;                 // the centre is the centre of mass of the cells above `threshold`
  double centre[3] = { 0., 0., 0. };
  double threshold = 0., delta = 1.;
  bflbm_radial() : bflbm_sample_store("radial trace", "bflbm_radial") {}
  size_t block() const { return (size_t)(1 + nq) * nbins; }
  size_t nbx() const { return (size_t)((G.plane + 255) / 256); }
  double* d_planes() const { return d_stage; }
  double* d_moments() const { return d_planes() + (size_t)nrep * G.nz * block(); }
  double* d_sums() const { return d_moments() + (com ? (size_t)nrep * kNTrace : 0); }
  double* d_fields() const { return d_sums() + (com ? (size_t)nrep * G.nz * nbx() * kNTrace : 0); }
  int record() override;
};

namespace {

// d = i - c taken to the minimum image of a periodic axis of n cells, in the order of the definition
__device__ __forceinline__ double radial_image(int i, double c, int n) {
  double d = (double)i - c;
  const double h = 0.5 * (double)n;
  if (d >= h) d = d - (double)n;
  else if (d < -h) d = d + (double)n;
  return d;
}

// grid (nz, replicas), 256 threads.  fields: the dense volumes, variable v of replica r at fields + r rep_stride +
// V.vol[v] comp_stride, [nz][ny][nx]; planes: [replica][z][1 + Q][nbins].  NV, the number of variables, is a template
// parameter: the site's variables are a register array of that size and the LDS holds NV + 4 rows.
template <int NV>
__global__ void __launch_bounds__(256) k_radial_shells(const double* __restrict__ fields, long long rep_stride, long long comp_stride,
                                                       const double* __restrict__ moments, double* __restrict__ planes,
                                                       int nx, int ny, int nz, double fx, double fy, double fz, double delta, int nbins,
                                                       FstatVars V, RadialTerms T, RadialRads R) {
  using namespace radial_limits;
  __shared__ double rows[NV + kMaxRad][kTile];
  __shared__ int sh_shell[kTile];
  __shared__ int sh_lo[4], sh_hi[4];
  __shared__ int sh_a[kMaxTerms], sh_b[kMaxTerms];
  const int tid = (int)threadIdx.x, z = (int)blockIdx.x, rep = (int)blockIdx.y;
  const int plane = nx * ny, nt = T.n, nitems = nt * nbins;
#pragma unroll
  for (int k = 0; k < kMaxTerms; ++k) if (tid == k) { sh_a[k] = T.a[k]; sh_b[k] = T.b[k]; }
  __syncthreads();
  // the items of this thread: (shell, term) = divmod(tid + 256 j, nt); the row offsets of its term, -1: the constant 1.0
  int shell_of[kMaxItems], off_a[kMaxItems], off_b[kMaxItems];
  double acc[kMaxItems];
#pragma unroll
  for (int j = 0; j < kMaxItems; ++j) {
    const int i = tid + 256 * j;
    const bool have = i < nitems;
    const int sh = have ? i / nt : -2, term = have ? i - sh * nt : 0;      // -2: in no tile's range
    const int a = sh_a[term], b = sh_b[term];
    shell_of[j] = sh; off_a[j] = a < 0 ? -1 : a * kTile; off_b[j] = b < 0 ? -1 : b * kTile;
    acc[j] = 0.;
  }
  double c[3];
  shape_centre(moments, rep, fx, fy, fz, c);
  const double dz = radial_image(z, c[2], nz);
  const double* vol[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) vol[v] = fields + (long long)rep * rep_stride + (long long)V.vol[v] * comp_stride + (long long)z * plane;
  const double* __restrict__ flat = &rows[0][0];

  for (int t0 = 0; t0 < plane; t0 += kTile) {
    const int s = t0 + tid;
    const bool in = s < plane;
    double x[NV][1];
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v][0] = in ? vol[v][s] : 0.;
    const int iy = s / nx, ix = s - iy * nx;
    const double dx = radial_image(ix, c[0], nx), dy = radial_image(iy, c[1], ny);
    const double r = sqrt((dx * dx + dy * dy) + dz * dz);
    const double q = r / delta;
    const int k = (in && q < (double)nbins) ? (int)q : -1;               // false for a NaN
#pragma unroll
    for (int v = 0; v < NV; ++v) rows[v][tid] = x[v][0];
#pragma unroll
    for (int u = 0; u < kMaxRad; ++u) {
      if (u < R.n) {
        double vx[1], vy[1], vz[1];
        fstat_pick<NV, 1>(x, R.v[u][0], vx);
        fstat_pick<NV, 1>(x, R.v[u][1], vy);
        fstat_pick<NV, 1>(x, R.v[u][2], vz);
        const double p = ((vx[0] * dx + vy[0] * dy) + vz[0] * dz) / r;
        rows[NV + u][tid] = r == 0. ? 0. : p;
      }
    }
    sh_shell[tid] = k;
    int lo = k < 0 ? 0x7fffffff : k, hi = k;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) { lo = min(lo, __shfl_xor(lo, w)); hi = max(hi, __shfl_xor(hi, w)); }
    if ((tid & 63) == 0) { sh_lo[tid >> 6] = lo; sh_hi[tid >> 6] = hi; }
    __syncthreads();
    lo = min(min(sh_lo[0], sh_lo[1]), min(sh_lo[2], sh_lo[3]));
    hi = max(max(sh_hi[0], sh_hi[1]), max(sh_hi[2], sh_hi[3]));
    const int cnt = min(kTile, plane - t0);
#pragma unroll
    for (int j = 0; j < kMaxItems; ++j) {
      const int mine = shell_of[j];
      if (mine >= lo && mine <= hi) {                                    // hi = -1 where the tile has no member
        const int oa = off_a[j], ob = off_b[j];
        double part = 0.;
#pragma unroll 8
        for (int m = 0; m < cnt; ++m) {
          if (sh_shell[m] == mine) {
            const double a = oa < 0 ? 1. : flat[oa + m];
            const double b = ob < 0 ? 1. : flat[ob + m];
            const double term = a * b;
            part += term;
          }
        }
        acc[j] += part;
      }
    }
    __syncthreads();                                                     // the next tile overwrites the rows
  }
  double* __restrict__ out = planes + ((long long)rep * nz + z) * nitems;
#pragma unroll
  for (int j = 0; j < kMaxItems; ++j) {
    const int i = tid + 256 * j;
    if (i < nitems) { const int sh = i / nt, term = i - sh * nt; out[term * nbins + sh] = acc[j]; }
  }
}

// grid (ceil((3 + (1 + Q) nbins) / 256), replicas): entry e < 3 of a replica's sample is the centre used, entry 3 + i the
// sum of entry i of the planes z = 0 .. nz-1 in sequence, from +0.0.  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_radial_finish(const double* __restrict__ planes, const double* __restrict__ moments,
                                                       double* __restrict__ out, double fx, double fy, double fz, int nz, int block) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= 3 + block) return;
  const int rep = (int)blockIdx.y;
  double v = 0.;
  if (e < 3) {
    double c[3];
    shape_centre(moments, rep, fx, fy, fz, c);
    v = e == 0 ? c[0] : (e == 1 ? c[1] : c[2]);
  } else {
    const double* __restrict__ p = planes + (long long)rep * nz * block + (e - 3);
    for (int z = 0; z < nz; ++z) v += p[(long long)z * block];
  }
  out[(long long)rep * (3 + block) + e] = v;
}

int radial_create(bflbm_ctx* c, bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                  int nrad, const int* rad_w, const int* rad_v, const double* centre, double threshold, double delta, int nbins,
                  int every, long long capacity, bflbm_radial** out) {
  using namespace radial_limits;
  const char* call = b ? "bflbm_batch_radial_create" : "bflbm_radial_create";
  if (field_refuse_args(call, source, 1, nvars, vars, npairs, pair_a, pair_b)) return 1;
  if (nrad < 0 || nrad > kMaxRad) return fail("%s: 0..%d radial terms (got %d)", call, kMaxRad, nrad);
  if (nrad > 0 && (!rad_w || !rad_v)) return fail("%s: null argument", call);
  for (int u = 0; u < nrad; ++u) {
    if (rad_w[u] < -1 || rad_w[u] >= nvars) return fail("%s: radial term %d: weight slot %d outside the %d variables (-1: none)", call, u, rad_w[u], nvars);
    for (int a = 0; a < 3; ++a)
      if (rad_v[3 * u + a] < 0 || rad_v[3 * u + a] >= nvars) return fail("%s: radial term %d: slot %d outside the %d variables", call, u, rad_v[3 * u + a], nvars);
  }
  if (centre && !(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2])))
    return fail("%s: the fixed centre is not finite", call);
  if (!centre && threshold != threshold) return fail("%s: the threshold is NaN (-INFINITY takes every cell)", call);
  if (!(std::isfinite(delta) && delta > 0.)) return fail("%s: delta must be finite and > 0 (got %g)", call, delta);
  if (nbins < 1 || nbins > kMaxBins) return fail("%s: 1..%d shells (got %d)", call, kMaxBins, nbins);
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_radial_create", "radial trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  if (G.nz > 65535) return fail("%s: nz = %d exceeds the 65535 planes of one launch", call, G.nz);

  std::unique_ptr<bflbm_radial> t(new bflbm_radial());
  const int nrep = b ? (int)b->ctx.size() : 1;
  t->G = G; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->nq = nvars + npairs + nrad; t->nbins = nbins;
  t->W = (G.nx * G.ny + kTile - 1) / kTile;
  t->com = !centre; t->threshold = threshold; t->delta = delta;
  if (centre) std::copy(centre, centre + 3, t->centre);
  t->fs = field_select(b != nullptr, source, nvars, vars);
  RadialTerms& T = t->terms;
  T.n = 0;
  for (int k = 0; k < kMaxTerms; ++k) { T.a[k] = -1; T.b[k] = -1; }
  T.n = 1;                                                               // the count: 1.0 * 1.0
  for (int v = 0; v < nvars; ++v) T.a[T.n++] = (signed char)v;
  for (int p = 0; p < npairs; ++p) { T.a[T.n] = (signed char)pair_a[p]; T.b[T.n++] = (signed char)pair_b[p]; }
  t->rads.n = nrad;
  for (int u = 0; u < kMaxRad; ++u) {
    for (int a = 0; a < 3; ++a) t->rads.v[u][a] = u < nrad ? rad_v[3 * u + a] : 0;
    if (u >= nrad) continue;
    if (rad_w[u] < 0) T.a[T.n++] = (signed char)(nvars + u);
    else { T.a[T.n] = (signed char)rad_w[u]; T.b[T.n++] = (signed char)(nvars + u); }
  }
  const size_t block = t->block();
  const size_t stage = (size_t)nrep * G.nz * block + (t->com ? (size_t)nrep * kNTrace * (1 + t->nbx() * (size_t)G.nz) : 0)
                     + (b ? (size_t)nrep * nvars * (size_t)t->nsites : 0);
  const std::string shape = " x (3 + " + std::to_string(1 + t->nq) + " x " + std::to_string(nbins) + ") shell sums";
  if (store_attach(t.get(), c, b, call, every, capacity, (size_t)nrep * (3 + block), stage, shape.c_str())) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// enqueue the observation, the centre and the two stages of the resident state into slot n; no host synchronisation
int bflbm_radial::record() {
  using namespace radial_limits;
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, d_fields(), "radial trace sample", &dense, &rep_stride)) return 1;
  if (com && trace_moments_launch(ctx, batch, G, nrep, threshold, d_sums(), d_moments(), stream)) return 1;
  const double* moments = com ? d_moments() : nullptr;
  const dim3 grid((unsigned)G.nz, (unsigned)nrep);
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_radial_shells<decltype(nv)::value>), grid, dim3(256), 0, stream, dense, rep_stride, nsites, moments, d_planes(),
                           G.nx, G.ny, G.nz, centre[0], centre[1], centre[2], delta, nbins, fs.vol, terms, rads);
      })) return fail("radial trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  const int blk = (int)block();
  hipLaunchKernelGGL(k_radial_finish, dim3((unsigned)((3 + blk + 255) / 256), (unsigned)nrep), dim3(256), 0, stream,
                     d_planes(), moments, store_slot(this), centre[0], centre[1], centre[2], G.nz, blk);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_radial_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                        int nrad, const int* rad_w, const int* rad_v, const double* centre_or_null, double threshold, double delta, int nbins,
                        int every, long long capacity, bflbm_radial** out) {
  if (!c || !vars || !out) return fail("bflbm_radial_create: null argument");
  return radial_create(c, nullptr, source, nvars, vars, npairs, pair_a, pair_b, nrad, rad_w, rad_v, centre_or_null, threshold, delta, nbins, every, capacity, out);
}
int bflbm_batch_radial_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                              int nrad, const int* rad_w, const int* rad_v, const double* centre_or_null, double threshold, double delta, int nbins,
                              int every, long long capacity, bflbm_radial** out) {
  if (!b || !vars || !out) return fail("bflbm_batch_radial_create: null argument");
  return radial_create(nullptr, b, source, nvars, vars, npairs, pair_a, pair_b, nrad, rad_w, rad_v, centre_or_null, threshold, delta, nbins, every, capacity, out);
}

int bflbm_radial_destroy(bflbm_radial* t) { return store_destroy(t); }
int bflbm_radial_sample(bflbm_radial* t) { return store_sample(t, "bflbm_radial"); }
int bflbm_radial_reset(bflbm_radial* t) { return store_reset(t, "bflbm_radial"); }
int bflbm_radial_count(const bflbm_radial* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_radial", nsamples, nreplicas); }
int bflbm_radial_read(bflbm_radial* t, long long first, long long count, double* rec, long long* steps) {
  return store_read(t, "bflbm_radial", first, count, rec, steps);
}

int bflbm_radial_geometry(const bflbm_radial* t, int* nsums, int* nbins, int* tile_sites, int* tiles_per_plane) {
  if (!t) return fail("bflbm_radial_geometry: null argument");
  if (nsums) *nsums = t->nq;
  if (nbins) *nbins = t->nbins;
  if (tile_sites) *tile_sites = radial_limits::kTile;
  if (tiles_per_plane) *tiles_per_plane = t->W;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_RADIAL_H_
