// bflbm_spectra.h -- the one transform layer of the structure factors (bflbm_sf.h, bflbm_sf_ring.h, bflbm_batch_sf.h)
// and the spectrum traces (bflbm_spectrum.h, bflbm_spectrum_ring.h): how observed fields become half spectra
// ("Transform layer").  Stated once here:
//   the hipFFT table, resolved with dlopen at first use (libbflbm.so itself does not depend on hipFFT);
//   the selection: the distinct variables of the pairs, ascending, a pair's slot being its variable's rank;
//   the dense transform of a lone context (hipfftPlan3d, one D2Z per distinct variable of the scratch buffer) or a batch
//     (one hipfftPlanMany D2Z over [B][nsel]) into hat[replica][spectrum][nk];
//   the slab transform of a ring of more than one slab.  Slab d owns the rows ky in [ny d / n, ny (d+1) / n) of the half
//     spectrum.  On every slab's stream, without a host synchronisation:
//       1. after the other slabs' `collected` (the last frame's h2 was taken): observe_launch into the scratch buffer, one
//          batched 2-D D2Z per distinct variable into h2[var][nzl][ny][nxc], the event `planes`;
//       2. after the other slabs' `planes`: k_spectrum_collect gathers the slab's rows of every plane of every slab into
//          zb[var][nz][nky][nxc], reading the sources' h2 in place, where every source is on the same device or
//          peer-mapped and neither the ring's transport nor BFLBM_RING_COPY_FALLBACK=1 asks for copies; strided (peer)
//          copies otherwise (the same doubles); the event `collected`;
//       3. batched Z2Z along z in place; then the kind's own work on zb (binning, or the pair product);
//   the pair product a^ conj(b^) / N into accumulators and their Hermitian expansion into the full fft-shifted spectrum.
// Included by bflbm.hip after bflbm_fieldsel.h and before the kinds (needs bflbm_ctx, bflbm_batch, bflbm_ring,
// ring_prepare_ref, ring_force_copies, recorder_stream, fields_observe, fields_observe_slab).
#ifndef BFLBM_SPECTRA_H_
#define BFLBM_SPECTRA_H_

#include <dlfcn.h>
#include <hipfft/hipfft.h>

struct SpectrumSrc { const double2* h2; int z0, nzl; };   // a source slab of the transpose, as k_spectrum_collect reads it

namespace {

// ---- the hipFFT table ------------------------------------------------------------------------------------------------------
struct FftApi {
  void* handle = nullptr;
  hipfftResult (*plan3d)(hipfftHandle*, int, int, int, hipfftType) = nullptr;
  hipfftResult (*plan_many)(hipfftHandle*, int, int*, int*, int, int, int*, int, int, hipfftType, int) = nullptr;
  hipfftResult (*set_stream)(hipfftHandle, hipStream_t) = nullptr;
  hipfftResult (*exec_d2z)(hipfftHandle, hipfftDoubleReal*, hipfftDoubleComplex*) = nullptr;
  hipfftResult (*exec_z2z)(hipfftHandle, hipfftDoubleComplex*, hipfftDoubleComplex*, int) = nullptr;
  hipfftResult (*destroy)(hipfftHandle) = nullptr;
  bool tried = false;
};
FftApi g_fft;

int load_fft() {
  if (g_fft.plan3d) return 0;
  if (g_fft.tried) return fail("hipFFT is not available (libhipfft.so.0 could not be loaded)");
  g_fft.tried = true;
  for (const char* name : {"libhipfft.so.0", "libhipfft.so", "/opt/rocm/lib/libhipfft.so.0"}) {
    g_fft.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (g_fft.handle) break;
  }
  if (!g_fft.handle) return fail("hipFFT is not available: %s", dlerror());
  g_fft.plan3d = (decltype(g_fft.plan3d))dlsym(g_fft.handle, "hipfftPlan3d");
  g_fft.plan_many = (decltype(g_fft.plan_many))dlsym(g_fft.handle, "hipfftPlanMany");
  g_fft.set_stream = (decltype(g_fft.set_stream))dlsym(g_fft.handle, "hipfftSetStream");
  g_fft.exec_d2z = (decltype(g_fft.exec_d2z))dlsym(g_fft.handle, "hipfftExecD2Z");
  g_fft.exec_z2z = (decltype(g_fft.exec_z2z))dlsym(g_fft.handle, "hipfftExecZ2Z");
  g_fft.destroy = (decltype(g_fft.destroy))dlsym(g_fft.handle, "hipfftDestroy");
  if (!g_fft.plan3d || !g_fft.plan_many || !g_fft.set_stream || !g_fft.exec_d2z || !g_fft.exec_z2z || !g_fft.destroy) {
    g_fft.plan3d = nullptr;
    return fail("hipFFT: missing symbols in the loaded library");
  }
  return 0;
}

// ---- the selection ---------------------------------------------------------------------------------------------------------
// the pairs as kernels take them: a, b the slots of the pair's spectra among one replica's; by value
struct SfPairs { int n; int a[32]; int b[32]; double scale[32]; };

struct SpectraSelection {
  FieldSelection fs;                // the distinct components of the pairs; what the observation writes
  std::vector<int> vars;            // those components, ascending: spectrum v of a replica is that of vars[v]
  int nspec = 0;                    // vars.size()
  SfPairs pairs;
};

// of accepted pairs (field_refuse_pair_vars); scale null: 1.0
SpectraSelection spectra_select(int source, int npairs, const int* var_a, const int* var_b, const double* scale) {
  SpectraSelection S;
  S.fs = field_select_pairs(source, npairs, var_a, var_b);
  for (int v = 0; v < BFLBM_NHYDRO_; ++v) if (S.fs.sel.mask & (1u << v)) S.vars.push_back(v);
  S.nspec = S.fs.sel.nsel;
  S.pairs.n = npairs;
  for (int p = 0; p < 32; ++p) {
    S.pairs.a[p] = p < npairs ? S.fs.sel.slot[var_a[p]] : 0;
    S.pairs.b[p] = p < npairs ? S.fs.sel.slot[var_b[p]] : 0;
    S.pairs.scale[p] = (p < npairs && scale) ? scale[p] : 1.0;
  }
  return S;
}

// ---- the dense transform: a lone context or a batch ----------------------------------------------------------------------
struct DenseSpectra {
  int device = 0;
  long long nsites = 0, nk = 0;     // sites, half-spectrum size
  hipfftHandle plan = nullptr;
  double* fields = nullptr;         // a batch: [nrep][nsel][nsites], what its observation writes
  double2* hat = nullptr;           // [nrep][nspec][nk]
  DenseSpectra() = default;
  DenseSpectra(const DenseSpectra&) = delete;
  DenseSpectra& operator=(const DenseSpectra&) = delete;
  ~DenseSpectra() {
    if (!plan && !fields && !hat) return;
    hipSetDevice(device);
    if (plan) g_fft.destroy(plan);
    if (fields) hipFree(fields);
    if (hat) hipFree(hat);
  }
};

// the owner: a lone context c or a batch b.  On failure D holds only what its destructor frees.
int dense_create(DenseSpectra& D, const char* call, const bflbm_ctx* c, const bflbm_batch* b, int nspec) {
  const Geo& G = c ? c->G : b->G;
  const int nx = G.nx, ny = G.ny, nz = G.nz, nrep = b ? (int)b->ctx.size() : 1;
  D.device = c ? c->dom.device : b->device;
  D.nsites = (long long)nx * ny * nz;
  D.nk = (long long)(nx / 2 + 1) * ny * nz;
  HIP_TRY(hipSetDevice(D.device));
  const size_t fb = b ? (size_t)nrep * nspec * D.nsites * sizeof(double) : 0, hb = (size_t)nrep * nspec * D.nk * sizeof(double2);
  hipError_t e = fb ? hipMalloc((void**)&D.fields, fb) : hipSuccess;
  if (e == hipSuccess) e = hipMalloc((void**)&D.hat, hb);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu + spectra %zu bytes): %s", call, fb, hb, hipGetErrorString(e));
  }
  hipfftResult fr;
  if (b) {
    int dims[3] = {nz, ny, nx};
    fr = g_fft.plan_many(&D.plan, 3, dims, nullptr, 1, (int)D.nsites, nullptr, 1, (int)D.nk, HIPFFT_D2Z, nrep * nspec);
  } else {
    fr = g_fft.plan3d(&D.plan, nz, ny, nx, HIPFFT_D2Z);
  }
  if (fr != HIPFFT_SUCCESS) {
    D.plan = nullptr;
    return fail("%s: the hipFFT plan failed for %d transform(s) of %d x %d x %d", call, b ? nrep * nspec : 1, nx, ny, nz);
  }
  return 0;
}

// enqueue the observation of `fs` and the transforms on the stream of the recorder's owner; no host synchronisation
int dense_run(DenseSpectra& D, const bflbm_recorder* rec, const FieldSelection& fs, const std::vector<int>& vars, const char* asker) {
  g_fft.set_stream(D.plan, recorder_stream(rec));      // the owner's stream may have been replaced since the last frame
  const double* dense;
  long long rep_stride;
  if (fields_observe(rec, fs, D.fields, asker, &dense, &rep_stride)) return 1;
  if (rec->batch) {
    if (g_fft.exec_d2z(D.plan, D.fields, (hipfftDoubleComplex*)D.hat) != HIPFFT_SUCCESS) return fail("%s: hipfftExecD2Z failed", asker);
  } else {
    for (size_t v = 0; v < vars.size(); ++v)
      if (g_fft.exec_d2z(D.plan, const_cast<double*>(dense) + (long long)vars[v] * D.nsites, (hipfftDoubleComplex*)(D.hat + (long long)v * D.nk)) != HIPFFT_SUCCESS)
        return fail("%s: hipfftExecD2Z failed", asker);
  }
  return 0;
}

// ---- the slab transform: a ring of more than one slab ----------------------------------------------------------------------
// The transpose, grid (ceil(nky nxc / 256), nz, variables) on the destination slab: plane z of variable v is the run of
// nky * nxc elements that starts at row ky0 of that plane in its source slab, copied 16 bytes per thread.  `src` lists
// the slabs in order (z0 ascending); the plane's source is found by a scan that is uniform over the workgroup.
__global__ void __launch_bounds__(256) k_spectrum_collect(const SpectrumSrc* __restrict__ src, int nsrc, double2* __restrict__ zb,
                                                          int ny, int nz, int ky0, int nky, int nxc) {
  const int z = (int)blockIdx.y, v = (int)blockIdx.z;
  int t = 0;
  while (t + 1 < nsrc && src[t + 1].z0 <= z) ++t;
  const SpectrumSrc S = src[t];
  const long long run = (long long)nky * nxc;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= run) return;
  // the table's pointers are device memory: said so, the load is a global one, not a flat one
  typedef double pair_t __attribute__((ext_vector_type(2)));
  typedef const pair_t __attribute__((address_space(1)))* global_pairs;
  const global_pairs from = (global_pairs)(S.h2 + (((long long)v * S.nzl + (z - S.z0)) * ny + ky0) * nxc);
  reinterpret_cast<pair_t*>(zb)[((long long)v * nz + z) * run + e] = from[e];
}

struct SlabSpectra {
  struct Slab {
    int device = 0, ky0 = 0, ky1 = 0;
    long long nk = 0;               // nz nky nxc
    hipfftHandle plan2d = nullptr, plan1d = nullptr;
    double2* h2 = nullptr;          // [var][nzl][ny][nxc]: the 2-D transforms of the own planes; the other slabs read it
    double2* zb = nullptr;          // [var][nz][nky][nxc]: the own rows of every plane, transformed along z in place
    SpectrumSrc* d_src = nullptr;   // [nslabs], in slab order
    bool reachable = false;         // every source is on this device or peer-mapped: k_spectrum_collect may read it in place
    hipEvent_t planes = nullptr;    // h2 is complete (recorded on the slab's stream) ...
    hipEvent_t collected = nullptr; // ... and this slab has taken its rows of every other slab's h2
  };
  int ny = 0, nz = 0, nxc = 0;
  std::vector<Slab> slab;
  SlabSpectra() = default;
  SlabSpectra(const SlabSpectra&) = delete;
  SlabSpectra& operator=(const SlabSpectra&) = delete;
  ~SlabSpectra() {
    for (Slab& q : slab) {
      hipSetDevice(q.device);
      if (q.plan2d) g_fft.destroy(q.plan2d);
      if (q.plan1d) g_fft.destroy(q.plan1d);
      for (void* p : {(void*)q.h2, (void*)q.zb, (void*)q.d_src}) if (p) hipFree(p);
      for (hipEvent_t e : {q.planes, q.collected}) if (e) hipEventDestroy(e);
    }
  }
};

// nspec spectra per frame.  On failure T holds only what its destructor frees.  Leaves the last slab's device selected.
int slab_create(SlabSpectra& T, const char* call, const bflbm_ring* g, int nspec) {
  const int n = (int)g->ctx.size();
  const Geo& G = g->ctx[0]->G;
  const int nx = G.nx, ny = G.ny, nz = G.nz, nxc = nx / 2 + 1;
  if (ny < n) return fail("%s: fewer rows (ny = %d) than slabs (%d)", call, ny, n);
  T.ny = ny; T.nz = nz; T.nxc = nxc;
  T.slab.resize((size_t)n);
  std::vector<SpectrumSrc> src((size_t)n);
  for (int d = 0; d < n; ++d) {
    const bflbm_ctx* c = g->ctx[d];
    SlabSpectra::Slab& q = T.slab[d];
    q.device = c->dom.device;
    q.ky0 = (int)((long long)ny * d / n); q.ky1 = (int)((long long)ny * (d + 1) / n);
    const int nky = q.ky1 - q.ky0;
    q.nk = (long long)nz * nky * nxc;
    HIP_TRY(hipSetDevice(q.device));
    const size_t hb = (size_t)nspec * c->nzl * ny * nxc * sizeof(double2), zb = (size_t)nspec * q.nk * sizeof(double2);
    hipError_t e = hipMalloc((void**)&q.h2, hb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.zb, zb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.d_src, (size_t)n * sizeof(SpectrumSrc));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail("%s: out of device memory on slab %d (plane spectra %zu + row spectra %zu bytes): %s", call, d, hb, zb, hipGetErrorString(e));
    }
    for (hipEvent_t* ev : {&q.planes, &q.collected}) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    int n2[2] = { ny, nx };
    if (g_fft.plan_many(&q.plan2d, 2, n2, nullptr, 1, ny * nx, nullptr, 1, ny * nxc, HIPFFT_D2Z, c->nzl) != HIPFFT_SUCCESS) {
      q.plan2d = nullptr;
      return fail("%s: the hipFFT plan failed for the %d planes of %d x %d of slab %d", call, c->nzl, nx, ny, d);
    }
    int n1[1] = { nz }, emb[1] = { nz };
    const int col = nky * nxc;                             // columns of one variable: the stride between the elements of a column
    if (g_fft.plan_many(&q.plan1d, 1, n1, emb, col, 1, emb, col, 1, HIPFFT_Z2Z, col) != HIPFFT_SUCCESS) {
      q.plan1d = nullptr;
      return fail("%s: the hipFFT plan failed for the %d columns of %d of slab %d", call, col, nz, d);
    }
    src[(size_t)d] = SpectrumSrc{ q.h2, c->dom.z0, c->nzl };
  }
  // the source table on every slab, and whether its kernels may read every source in place (the rule of ring_copy)
  for (int d = 0; d < n; ++d) {
    SlabSpectra::Slab& q = T.slab[d];
    HIP_TRY(hipSetDevice(q.device));
    HIP_TRY(hipMemcpy(q.d_src, src.data(), (size_t)n * sizeof(SpectrumSrc), hipMemcpyHostToDevice));
    q.reachable = true;
    for (int s = 0; s < n; ++s) {
      const int pd = T.slab[s].device;
      if (pd == q.device) continue;
      int can = 0; hipDeviceCanAccessPeer(&can, q.device, pd);
      bool ok = false;
      if (can) { const hipError_t pe = hipDeviceEnablePeerAccess(pd, 0); ok = (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled); }
      (void)hipGetLastError();
      q.reachable = q.reachable && ok;
    }
  }
  return 0;
}

// Enqueue one frame of the ring's resident state: steps 1 to 3 above, then then(d, zb, nk, stream) with slab d's device
// selected hands its transformed rows to the kind, slab by slab.  No host synchronisation beyond the centre-of-mass sum
// of ring_prepare_ref, which hydrovs under a reference state needs.
template <class Then>
int slab_run(SlabSpectra& T, bflbm_ring* g, const FieldSelection& fs, const std::vector<int>& vars, const char* asker, Then then) {
  const int n = (int)g->ctx.size(), ny = T.ny, nz = T.nz, nxc = T.nxc;
  const size_t nv = vars.size();
  if (fs.source != 1 && ring_prepare_ref(g)) return 1;                // the global centre of mass: the slabs' own prepare_ref is then a no-op
  const bool in_place = !ring_force_copies() && g->transport == 0;
  // 1. observe + 2-D transforms of the own planes
  for (int k = 0; k < n; ++k) {
    bflbm_ctx* c = g->ctx[k];
    SlabSpectra::Slab& q = T.slab[k];
    HIP_TRY(hipSetDevice(q.device));
    for (int d = 0; d < n; ++d) if (d != k) HIP_TRY(hipStreamWaitEvent(c->stream, T.slab[d].collected, 0));   // the last frame's h2 was taken
    const double* dense;                                  // [comp][z local][y][x]
    if (fields_observe_slab(c, fs, asker, &dense)) return 1;
    const long long nloc = (long long)c->nzl * c->G.dplane;
    g_fft.set_stream(q.plan2d, c->stream);
    for (size_t v = 0; v < nv; ++v)
      if (g_fft.exec_d2z(q.plan2d, const_cast<double*>(dense) + (long long)vars[v] * nloc,
                         (hipfftDoubleComplex*)(q.h2 + (long long)v * c->nzl * ny * nxc)) != HIPFFT_SUCCESS)
        return fail("%s: hipfftExecD2Z (planes of slab %d) failed", asker, k);
    HIP_TRY(hipEventRecord(q.planes, c->stream));
  }
  // 2. the transpose and 3. the z transforms of the own rows
  for (int d = 0; d < n; ++d) {
    bflbm_ctx* c = g->ctx[d];
    SlabSpectra::Slab& q = T.slab[d];
    const int nky = q.ky1 - q.ky0;
    const long long run = (long long)nky * nxc;
    HIP_TRY(hipSetDevice(q.device));
    for (int s = 0; s < n; ++s) if (s != d) HIP_TRY(hipStreamWaitEvent(c->stream, T.slab[s].planes, 0));
    if (in_place && q.reachable) {
      hipLaunchKernelGGL(k_spectrum_collect, dim3((unsigned)((run + 255) / 256), (unsigned)nz, (unsigned)nv), dim3(256), 0, c->stream,
                         q.d_src, n, q.zb, ny, nz, q.ky0, nky, nxc);
      HIP_TRY(hipGetLastError());
    } else {
      for (int s = 0; s < n; ++s) {
        const bflbm_ctx* cs = g->ctx[s];
        for (size_t v = 0; v < nv; ++v) {
          const double2* from = T.slab[s].h2 + ((long long)v * cs->nzl * ny + q.ky0) * nxc;            // plane 0 of slab s, row ky0
          double2* to = q.zb + ((long long)v * nz + cs->dom.z0) * run;                                  // global plane z0_s
          HIP_TRY(hipMemcpy2DAsync(to, (size_t)run * sizeof(double2), from, (size_t)ny * nxc * sizeof(double2),
                                   (size_t)run * sizeof(double2), (size_t)cs->nzl, hipMemcpyDefault, c->stream));
        }
      }
    }
    HIP_TRY(hipEventRecord(q.collected, c->stream));
    g_fft.set_stream(q.plan1d, c->stream);
    for (size_t v = 0; v < nv; ++v) {
      hipfftDoubleComplex* p = (hipfftDoubleComplex*)(q.zb + (long long)v * q.nk);
      if (g_fft.exec_z2z(q.plan1d, p, p, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail("%s: hipfftExecZ2Z (columns of slab %d) failed", asker, d);
    }
    if (then(d, q.zb, q.nk, c->stream)) return 1;
  }
  return 0;
}

// ---- the pair product and the expansion ------------------------------------------------------------------------------------
// grid (ceil(nk / 256), npairs, replicas): acc[r][p][k] += scale[p] * a^(k) conj(b^(k)) / N over the half spectrum, the
// spectra of replica r at hat[r][nspec][nk]
__global__ void __launch_bounds__(256) k_sf_accumulate(const double2* __restrict__ hat, double2* __restrict__ acc,
                                                       long long nk, int nspec, SfPairs P, double inv_n) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nk) return;
  const int p = blockIdx.y;
  const double2* __restrict__ mine = hat + (long long)blockIdx.z * nspec * nk;
  const double2 a = mine[(long long)P.a[p] * nk + k], b = mine[(long long)P.b[p] * nk + k];
  const double s = P.scale[p];
  const double ar = s * a.x, ai = s * a.y;
  const long long at = ((long long)blockIdx.z * P.n + p) * nk + k;
  double2 v = acc[at];
  v.x += (ar * b.x + ai * b.y) * inv_n;
  v.y += (ai * b.x - ar * b.y) * inv_n;
  acc[at] = v;
}

int sf_accumulate_launch(const double2* hat, double2* acc, long long nk, int nspec, const SfPairs& P, int nrep, double inv_n, hipStream_t stream) {
  const dim3 grid((unsigned)((nk + 255) / 256), (unsigned)P.n, (unsigned)nrep);
  hipLaunchKernelGGL(k_sf_accumulate, grid, dim3(256), 0, stream, hat, acc, nk, nspec, P, inv_n);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Site s of the full fft-shifted spectrum [z][y][x] (k = 0 at (nz/2, ny/2, nx/2); shifted index i holds frequency index
// (i - n/2) mod n, numpy's shift by n//2): where its value lies in the half spectrum [kz][ky][kx'], whether it is the
// conjugate of that entry (S(-k) = conj(S(k)) for real fields), and whether it is k = 0.
struct SfSite { long long at; bool conj, zero; };
__host__ __device__ inline SfSite sf_site(long long s, int nx, int ny, int nz) {
  const int xs = (int)(s % nx), ys = (int)((s / nx) % ny), zs = (int)(s / ((long long)nx * ny));
  int kx = xs - nx / 2; if (kx < 0) kx += nx;
  int ky = ys - ny / 2; if (ky < 0) ky += ny;
  int kz = zs - nz / 2; if (kz < 0) kz += nz;
  const int nxc = nx / 2 + 1;
  const bool own = kx < nxc;
  const int mx = own ? kx : nx - kx, my = own ? ky : (ny - ky) % ny, mz = own ? kz : (nz - kz) % nz;
  return SfSite{ ((long long)mz * ny + my) * nxc + mx, !own, kx == 0 && ky == 0 && kz == 0 };
}
// the value of that site from the summed accumulator entry (re, im); what: 0 |S|, 1 Re S, 2 Im S
__host__ __device__ inline double sf_value(double re, double im, const SfSite& K, double inv, int what, int zero_avg) {
  if (K.conj) im = -im;
  re *= inv; im *= inv;
  if (zero_avg && K.zero) { re = 0.; im = 0.; }
  return (what == 0) ? hypot(re, im) : (what == 1 ? re : im);
}

// grid (ceil(n / 256), npairs): the full fft-shifted mean spectrum out[p][z][y][x] from acc[nrep][npairs][nk], of replica
// `replica` (inv = 1 / frames) or, replica < 0, of the ensemble: the nrep accumulators of the (pair, k) added in the
// order 0 ... nrep-1, times inv = 1 / (nrep frames).  |S| is that of the complex mean.
__global__ void __launch_bounds__(256) k_sf_expand(const double2* __restrict__ acc, double* __restrict__ out,
                                                   int nx, int ny, int nz, int npairs, int nrep, int replica,
                                                   double inv, int what, int zero_avg) {
  const long long n = (long long)nx * ny * nz;
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int p = blockIdx.y;
  const SfSite K = sf_site(s, nx, ny, nz);
  const long long nk = (long long)(nx / 2 + 1) * ny * nz;
  const long long at = (long long)p * nk + K.at;
  double re, im;
  if (replica >= 0) {
    const double2 v = acc[(long long)replica * npairs * nk + at];
    re = v.x; im = v.y;
  } else {
    re = 0.; im = 0.;
    for (int r = 0; r < nrep; ++r) { const double2 v = acc[(long long)r * npairs * nk + at]; re += v.x; im += v.y; }
  }
  out[(long long)p * n + s] = sf_value(re, im, K, inv, what, zero_avg);
}

// the stream of an accumulator's owner, or the null stream once it is gone: detaching waited for everything enqueued
inline hipStream_t sf_stream(const bflbm_recorder* s) { return recorder_attached(s) ? recorder_stream(s) : nullptr; }

// the expansion into `out` on the device ([npairs][sites]) and its download to dst on the host; waits for the stream
int sf_expand_get(const double2* acc, double* out, double* dst, int nx, int ny, int nz, int npairs, int nrep, int replica,
                  long long frames, int what, int zero_avg, hipStream_t stream) {
  const long long n = (long long)nx * ny * nz;
  const double inv = 1.0 / (replica < 0 ? (double)nrep * (double)std::max(frames, 1LL) : (double)std::max(frames, 1LL));
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)npairs);
  hipLaunchKernelGGL(k_sf_expand, grid, dim3(256), 0, stream, acc, out, nx, ny, nz, npairs, nrep, replica, inv, what, zero_avg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, out, (size_t)npairs * n * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

}  // namespace

#endif  // BFLBM_SPECTRA_H_
