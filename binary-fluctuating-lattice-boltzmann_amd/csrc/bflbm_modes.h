// bflbm_modes.h -- mode traces: the complex Fourier amplitudes a^(m, t) of chosen hydrodynamic variables at chosen
// integer wavevectors, recorded on the device as a time series for a lone single-slab context or every replica of a
// batch (include/bflbm.h, "Mode traces": the definition and the order of every sum are stated there and only there).
// The spectrum trace keeps Re(a^ conj b^) summed over bins; time correlations need the amplitudes of single wavevectors
// at consecutive steps, and a full hipFFT per variable and step for a dozen wavevectors is the wrong tool.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   batch_observe_launch into the trace's [B][nsel][n] / observe_launch into the scratch buffer,
//   k_modes_project                 stage 1: per tile of 2048 consecutive sites of a dense plane and replica, for every
//                                   (variable, wavevector) the sum of a(x, y) T_nx[jx] T_ny[jy], threads striding the
//                                   tile, the tree of block_reduce, into [replica][z][tile][var][mode][2],
//   k_modes_finish                  stage 2: per (variable, wavevector, replica) the tiles of a plane in tile order,
//                                   times T_nz[jz], the planes in the sequence z = 0 .. nz-1, into the slot.
// The planes are the last sum, so that a ring of z-slabs can follow the way bflbm_ring_trace_create did.  No atomics,
// no scratch.  Not built on purpose: reading the populations in stage 1 to skip the dense intermediate; it would save
// traffic for hydrovsbar only, whose observation is a plain moment sum.
// The lifecycle and the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by
// bflbm.hip after bflbm_batch_sf.h (needs bflbm_ctx, bflbm_batch, FieldSelection, fields_observe, field_dispatch_nv).
#ifndef BFLBM_MODES_H_
#define BFLBM_MODES_H_

#include <cmath>
#include <memory>
#include <string>
#include <vector>

// ---- the phase tables: host code that needs nothing of the library (a stand-alone program may include this part alone) ----
namespace modes_tables {

constexpr int kTile = 2048;          // sites per workgroup of stage 1: 8 per thread.  An untimed heuristic.
constexpr int kPerThread = kTile / 256;
constexpr int kTabMax = 2304;        // entries of the x and y half tables (nx/2 + 1) + (ny/2 + 1) that stage 1 keeps in LDS
constexpr int kMaxVars = 8, kMaxModes = 64;

// T_n[j] = (cos(2 pi j / n), -sin(2 pi j / n)), j = 0 .. n-1, table[j][2].  The angle is reduced to an octant in
// integers, so the quarter points are exact, and the upper half is the conjugate of the lower by construction.
inline void phases(int n, double* table) {
  const long double half_pi = 1.57079632679489661923132169163975144L;
  for (int j = 0; 2 * j <= n; ++j) {
    const long long q4 = 4LL * j;
    const int quad = (int)(q4 / n);                      // 0, 1 or 2 (j <= n/2)
    const long long u = q4 % n;                          // the angle inside the quadrant is (pi/2) u / n
    long double c, s;
    if (2 * u <= n) { const long double a = half_pi * (long double)u / (long double)n; c = cosl(a); s = sinl(a); }
    else { const long double b = half_pi * (long double)(n - u) / (long double)n; c = sinl(b); s = cosl(b); }
    if (u == 0) { c = 1.L; s = 0.L; }
    long double co, si;
    if (quad == 0) { co = c; si = s; } else if (quad == 1) { co = -s; si = c; } else { co = -c; si = -s; }
    table[2 * j] = (double)co;
    table[2 * j + 1] = -(double)si;
  }
  for (int j = n / 2 + 1; j < n; ++j) { table[2 * j] = table[2 * (n - j)]; table[2 * j + 1] = -table[2 * (n - j) + 1]; }
}

inline int reduce(int m, int n) { const int r = m % n; return r < 0 ? r + n : r; }

}  // namespace modes_tables

#ifndef BFLBM_MODES_TABLES_ONLY

// where the trace's variables lie among the dense volumes of one replica
struct ModesVars { int n; int vol[modes_tables::kMaxVars]; };
// per wavevector: mx mod nx, my mod ny, (256 mx) mod nx, ((256 / nx) my) mod ny: what advances the phase indices
struct ModesStep { int mx, my, dx, dy; };

struct bflbm_modes : bflbm_sample_store {    // d_rec [capacity][nrep][nvars][nmodes][2], d_stage [nrep][nz][tiles][nvars][nmodes][2]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar
  int nmodes = 0, tiles = 0;
  ModesVars vars;                   // fs.nvars and fs.vol as the projection kernel takes them
  double* fields = nullptr;         // a batch: [nrep][nsel][nsites]
  double2* d_tab = nullptr;         // T_nx[0 .. nx/2], T_ny[0 .. ny/2], T_nz[0 .. nz-1]
  ModesStep* d_step = nullptr;      // [nmodes]
  int* d_mz = nullptr;              // [nmodes]: mz mod nz
  bflbm_modes() : bflbm_sample_store("mode trace", "bflbm_modes") {}
  ~bflbm_modes() override {
    for (void* p : {(void*)fields, (void*)d_tab, (void*)d_step, (void*)d_mz}) if (p) hipFree(p);
  }
  int record() override;
};

namespace {

// entry j of a full table kept as its lower half t[0 .. n/2]: the upper half is the conjugate
__device__ __forceinline__ double2 modes_phase(const double2* t, int j, int n) {
  const bool up = 2 * j > n;
  double2 v = t[up ? n - j : j];
  if (up) v.y = -v.y;
  return v;
}

// Stage 1, grid (tiles, nz, B).  Thread t takes the sites t, t + 256, ... of the tile in that order; a site's values are
// loaded once and kept for every wavevector.  Per wavevector the phase indices jx = (mx x) mod nx and jy = (my y) mod ny
// are formed once for the thread's first site and advance by additions and a conditional subtraction; the xy phase of a
// (site, wavevector) is formed once and applied to all variables.  The 256 partial sums of a wavevector are added in the
// order of block_reduce's tree, all variables at once.  NV, the number of variables, is a template parameter: the accumulators
// and the site values are register arrays, and a run-time count costs a select per (site, variable, wavevector).
template <int NV>
__global__ void __launch_bounds__(256) k_modes_project(const double* __restrict__ fields, long long rep_stride, long long nsites,
                                                       const double2* __restrict__ tab, const ModesStep* __restrict__ step,
                                                       double* __restrict__ partial, int nx, int ny, int nmodes, ModesVars V) {
  using namespace modes_tables;
  __shared__ double2 T[kTabMax];
  __shared__ double xa[2 * NV][128];                     // level 128 of the tree: waves 2, 3 to waves 0, 1
  __shared__ double xb[2 * NV][64];                      // level 64: wave 1 to wave 0
  const int tid = (int)threadIdx.x;
  const int hx = nx / 2 + 1, hy = ny / 2 + 1;
  for (int i = tid; i < hx + hy; i += 256) T[i] = tab[i];
  const double2* Tx = T;
  const double2* Ty = T + hx;
  const int plane = nx * ny;
  const int s0 = (int)blockIdx.x * kTile + tid;
  const double* __restrict__ F = fields + (long long)blockIdx.z * rep_stride + (long long)blockIdx.y * plane;
  double a[kPerThread][NV];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int s = s0 + 256 * i;
#pragma unroll
    for (int v = 0; v < NV; ++v) a[i][v] = s < plane ? F[(long long)V.vol[v] * nsites + s] : 0.;
  }
  // which of the thread's strides of 256 sites carry one row more than 256 / nx
  const int x0 = s0 % nx, y0 = s0 / nx, rx = 256 % nx;
  unsigned carry = 0;
  {
    int x = x0;
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) { x += rx; if (x >= nx) { x -= nx; carry |= 1u << i; } }
  }
  __syncthreads();
  double* __restrict__ out = partial + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * ((long long)NV * nmodes * 2);
  for (int m = 0; m < nmodes; ++m) {
    const ModesStep M = step[m];
    int jx = (M.mx * x0) % nx, jy = (int)(((long long)M.my * y0) % ny);
    double re[NV], im[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) { re[v] = 0.; im[v] = 0.; }
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const double2 px = modes_phase(Tx, jx, nx), py = modes_phase(Ty, jy, ny);
      const double pr = px.x * py.x - px.y * py.y, pi = px.x * py.y + px.y * py.x;
#pragma unroll
      for (int v = 0; v < NV; ++v) { re[v] += a[i][v] * pr; im[v] += a[i][v] * pi; }
      jx += M.dx; if (jx >= nx) jx -= nx;
      jy += M.dy; if (jy >= ny) jy -= ny;
      if (carry & (1u << i)) { jy += M.my; if (jy >= ny) jy -= ny; }
    }
    // the tree of block_reduce, v[t] += v[t + w] for w = 128, 64, ..., 1, with the same operands in the same order: the upper
    // two waves hand their sums to the lower two through LDS, wave 1 hands its to wave 0, and wave 0 finishes by lane
    // shifts (lane t adds lane t + w; the lanes t >= w hold values no later level reads).  Two barriers per wavevector;
    // xa of the next wavevector is written after the second barrier of this one, xb after its first, so nothing is
    // overwritten while it is read.
    if (tid >= 128) {
#pragma unroll
      for (int v = 0; v < NV; ++v) { xa[2 * v][tid - 128] = re[v]; xa[2 * v + 1][tid - 128] = im[v]; }
    }
    __syncthreads();
    if (tid < 128) {
#pragma unroll
      for (int v = 0; v < NV; ++v) { re[v] += xa[2 * v][tid]; im[v] += xa[2 * v + 1][tid]; }
      if (tid >= 64) {
#pragma unroll
        for (int v = 0; v < NV; ++v) { xb[2 * v][tid - 64] = re[v]; xb[2 * v + 1][tid - 64] = im[v]; }
      }
    }
    __syncthreads();
    if (tid < 64) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        re[v] += xb[2 * v][tid]; im[v] += xb[2 * v + 1][tid];
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) { re[v] += __shfl_down(re[v], w); im[v] += __shfl_down(im[v], w); }
        if (tid == 0) {
          double* o = out + ((long long)v * nmodes + m) * 2;
          o[0] = re[v]; o[1] = im[v];
        }
      }
    }
  }
}

// Stage 2, grid (nvars * nmodes, B), 256 threads: in rounds of 256 planes, thread t adds the tiles of plane z = base + t
// in tile order and multiplies the sum by T_nz[(mz z) mod nz]; thread 0 then adds the round's planes in sequence.
// out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_modes_finish(const double* __restrict__ partial, const double2* __restrict__ tz,
                                                      const int* __restrict__ mzs, double* __restrict__ out,
                                                      int nz, int tiles, int nmodes) {
  __shared__ double2 sh[256];
  const int tid = (int)threadIdx.x;
  const long long nvm = gridDim.x;                                      // nvars * nmodes
  const int mz = mzs[blockIdx.x % nmodes];
  const double* __restrict__ mine = partial + (long long)blockIdx.y * nz * tiles * nvm * 2 + (long long)blockIdx.x * 2;
  double re = 0., im = 0.;
  for (int base = 0; base < nz; base += 256) {
    const int z = base + tid;
    if (z < nz) {
      double sr = 0., si = 0.;
      const double* __restrict__ p = mine + (long long)z * tiles * nvm * 2;
      for (int t = 0; t < tiles; ++t) { sr += p[0]; si += p[1]; p += nvm * 2; }
      const double2 b = tz[(int)(((long long)mz * z) % nz)];
      sh[tid] = make_double2(sr * b.x - si * b.y, sr * b.y + si * b.x);
    }
    __syncthreads();
    if (tid == 0) {
      const int cnt = nz - base < 256 ? nz - base : 256;
      for (int i = 0; i < cnt; ++i) { re += sh[i].x; im += sh[i].y; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = out + ((long long)blockIdx.y * nvm + blockIdx.x) * 2;
    o[0] = re; o[1] = im;
  }
}

int modes_create(bflbm_ctx* c, bflbm_batch* b, int nvars, const int* vars, int lb_hydrovars, int nmodes, const int* modes,
                 int every, long long capacity, bflbm_modes** out) {
  using namespace modes_tables;
  const char* call = b ? "bflbm_batch_modes_create" : "bflbm_modes_create";
  const int source = lb_hydrovars ? 1 : 0;
  if (field_refuse_args(call, source, 1, nvars, vars, 0, nullptr, nullptr)) return 1;
  if (nmodes < 1 || nmodes > kMaxModes) return fail("%s: 1..%d wavevectors (got %d)", call, kMaxModes, nmodes);
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_modes_create", "mode trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  const Geo& G = c ? c->G : b->G;
  const int nx = G.nx, ny = G.ny, nz = G.nz;
  const int hx = nx / 2 + 1, hy = ny / 2 + 1;
  if (hx + hy > kTabMax)
    return fail("%s: the x and y phase tables of %d x %d x %d have %d + %d entries, more than the %d the projection kernel keeps in LDS",
                call, nx, ny, nz, hx, hy, kTabMax);
  if (nz > 65535) return fail("%s: nz = %d exceeds the 65535 planes of one launch", call, nz);
  HIP_TRY(hipSetDevice(c ? c->dom.device : b->device));

  std::unique_ptr<bflbm_modes> t(new bflbm_modes());
  const int nrep = c ? 1 : (int)b->ctx.size();
  t->nx = nx; t->ny = ny; t->nz = nz; t->nsites = (long long)nx * ny * nz;
  t->nmodes = nmodes;
  t->tiles = (nx * ny + kTile - 1) / kTile;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  static_assert(kMaxVars == fstat_limits::kMaxVars, "ModesVars holds the selection's volumes");
  t->vars.n = nvars;
  std::copy(t->fs.vol.vol, t->fs.vol.vol + kMaxVars, t->vars.vol);

  std::vector<double> tab((size_t)2 * (hx + hy + nz)), full;
  const int dims[3] = {nx, ny, nz};
  size_t at = 0;
  for (int d = 0; d < 3; ++d) {
    full.assign((size_t)2 * dims[d], 0.);
    phases(dims[d], full.data());
    const int keep = d == 0 ? hx : (d == 1 ? hy : nz);
    std::copy(full.begin(), full.begin() + 2 * keep, tab.begin() + at);
    at += (size_t)2 * keep;
  }
  std::vector<ModesStep> step((size_t)nmodes);
  std::vector<int> mz((size_t)nmodes);
  for (int m = 0; m < nmodes; ++m) {
    ModesStep& S = step[(size_t)m];
    S.mx = reduce(modes[3 * m], nx); S.my = reduce(modes[3 * m + 1], ny); mz[(size_t)m] = reduce(modes[3 * m + 2], nz);
    S.dx = (int)((256LL * S.mx) % nx);
    S.dy = (int)(((long long)(256 / nx) * S.my) % ny);
  }

  const size_t fb = b ? (size_t)nrep * nvars * t->nsites * sizeof(double) : 0;
  const size_t tb = tab.size() * sizeof(double), sb = step.size() * sizeof(ModesStep), zb = mz.size() * sizeof(int);
  const size_t per = (size_t)nrep * nvars * nmodes * 2;
  const size_t stage = (size_t)nrep * nz * t->tiles * nvars * nmodes * 2;
  hipError_t e = fb ? hipMalloc((void**)&t->fields, fb) : hipSuccess;
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_tab, tb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_step, sb);
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_mz, zb);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu + phase tables %zu + wavevectors %zu + %zu bytes; then records %zu x %lld + tile sums %zu): %s",
                call, fb, tb, sb, zb, per * sizeof(double), capacity, stage * sizeof(double), hipGetErrorString(e));
  }
  HIP_TRY(hipMemcpy(t->d_tab, tab.data(), tb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t->d_step, step.data(), sb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t->d_mz, mz.data(), zb, hipMemcpyHostToDevice));
  const std::string shape = " x " + std::to_string(nvars) + " variables x " + std::to_string(nmodes) + " wavevectors";
  if (store_attach(t.get(), c, b, call, every, capacity, per, stage, shape.c_str())) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// enqueue the observation and the two stages of the resident state into slot n; no host synchronisation
int bflbm_modes::record() {
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "mode trace sample", &dense, &rep_stride)) return 1;
  const dim3 grid((unsigned)tiles, (unsigned)nz, (unsigned)nrep);
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_modes_project<decltype(nv)::value>), grid, dim3(256), 0, stream, dense, rep_stride, nsites, d_tab, d_step, d_stage, nx, ny, nmodes, vars);
      })) return fail("mode trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_modes_finish, dim3((unsigned)(fs.nvars * nmodes), (unsigned)nrep), dim3(256), 0, stream,
                     d_stage, d_tab + (nx / 2 + 1) + (ny / 2 + 1), d_mz, store_slot(this), nz, tiles, nmodes);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_modes_create(bflbm_ctx* c, int nvars, const int* vars, int lb_hydrovars, int nmodes, const int* modes,
                       int every, long long capacity, bflbm_modes** out) {
  if (!c || !vars || !modes || !out) return fail("bflbm_modes_create: null argument");
  return modes_create(c, nullptr, nvars, vars, lb_hydrovars, nmodes, modes, every, capacity, out);
}
int bflbm_batch_modes_create(bflbm_batch* b, int nvars, const int* vars, int lb_hydrovars, int nmodes, const int* modes,
                             int every, long long capacity, bflbm_modes** out) {
  if (!b || !vars || !modes || !out) return fail("bflbm_batch_modes_create: null argument");
  return modes_create(nullptr, b, nvars, vars, lb_hydrovars, nmodes, modes, every, capacity, out);
}

int bflbm_modes_destroy(bflbm_modes* t) { return store_destroy(t); }
int bflbm_modes_sample(bflbm_modes* t) { return store_sample(t, "bflbm_modes"); }
int bflbm_modes_reset(bflbm_modes* t) { return store_reset(t, "bflbm_modes"); }
int bflbm_modes_count(const bflbm_modes* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_modes", nsamples, nreplicas); }
int bflbm_modes_read(bflbm_modes* t, long long first, long long count, double* amp, long long* steps) {
  return store_read(t, "bflbm_modes", first, count, amp, steps);
}

int bflbm_modes_geometry(const bflbm_modes* t, int* nvars, int* nmodes, int* tiles_per_plane, int* tile_sites) {
  if (!t) return fail("bflbm_modes_geometry: null argument");
  if (nvars) *nvars = t->fs.nvars;
  if (nmodes) *nmodes = t->nmodes;
  if (tiles_per_plane) *tiles_per_plane = t->tiles;
  if (tile_sites) *tile_sites = modes_tables::kTile;
  return 0;
}

int bflbm_modes_phases(int n, double* table) {
  if (!table) return fail("bflbm_modes_phases: null argument");
  if (n < 1) return fail("bflbm_modes_phases: n must be >= 1 (got %d)", n);
  modes_tables::phases(n, table);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_MODES_TABLES_ONLY

#endif  // BFLBM_MODES_H_
