// bflbm_batch_sf.h -- ensemble structure factors: S(k) of every replica of a batch in one batched pass
// (include/bflbm.h, "Ensemble structure factors").  One accumulator per bflbm_sf costs a batch of B replicas B observation
// launches, B x (distinct variables) transforms and B accumulation launches per frame; here a frame is, on the batch's
// stream and without a host synchronisation,
//   k_observe_batch        the selected components of hydrovs (or hydrovsbar) of all replicas, densely [B][nsel][n],
//   one hipfftExecD2Z      of a hipfftPlanMany plan with batch = B * nsel,                  spectra    [B][nsel][nk],
//   k_sf_accumulate_batch  a^ conj(b^) / N of every pair and replica,                       accumulators [B][npairs][nk].
// The accumulator owns all four buffers; of the replicas only rho / phi are written, by one k_density_batch launch, when
// hydrovs is observed and some replica's densities are not those of its resident state.
// k_observe_batch computes, per site, what k_observe computes (the same device functions in the same order, no injected
// noise, no reference state), so the stacked getters bflbm_batch_get_hydrovs / _hydrovsbar return the doubles of the views'.
// The link to the batch, the every-count and the detaching are those of bflbm_recorder.h.
// Included by bflbm.hip after bflbm_batch.h, bflbm_fieldsel.h, bflbm_sf.h and bflbm_trace.h (needs bflbm_batch, FftApi,
// SfPairs, ObsSel, field_select_pairs).
#ifndef BFLBM_BATCH_SF_H_
#define BFLBM_BATCH_SF_H_

namespace {

// grid (plane blocks, nz, B): WHAT 0 hydrovsbar (LBM_binary.H:315-340), 2 hydrovs (:196-295) of replica blockIdx.z,
// out[(r * nsel + slot) * n + site]
template <int WHAT>
__global__ void __launch_bounds__(256) k_observe_batch(const BatchRec* __restrict__ recs, double* __restrict__ out, Geo G, int k, ObsSel sel) {
  static_assert(WHAT == 0 || WHAT == 2, "hydrovsbar or hydrovs");
  __shared__ double ntab[WHAT != 0 ? BFLBM_NORMAL_TABLE_N : 4];
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const DevParams& P = batch_params(R);
  if (WHAT != 0) d_load_normal_table(ntab, P.noise_on != 0);
  const int p0 = 0;
  BFLBM_SITE_FROM_BLOCK();
  const double* __restrict__ S = R->S[R->cur0 ^ (k & 1)];
  SiteIdx I; site_index(G, x, y, p, I);
  double fs[Q], gs[Q];
  pull_site(S, G, I, fs, gs);
  const long long n = (long long)G.nzs * G.dplane;                    // batches: no halo planes
  double* __restrict__ o = out + (long long)blockIdx.z * sel.nsel * n + ((long long)p * G.dplane + (long long)y * G.nx + x);
  const double r = d_density(fs), ph = d_density(gs);
  if (WHAT == 0) {
    double mf[Q], mg[Q];
    d_moments(fs, mf); d_moments(gs, mg);
    double h[BFLBM_NHYDROBAR];
    h[0] = r; h[1] = ph;
    const bool okf = fabs(mf[0]) > (double)FLT_EPSILON, okg = fabs(mg[0]) > (double)FLT_EPSILON;
#pragma unroll
    for (int a = 1; a <= 3; ++a) { h[a + 1] = okf ? mf[a] / mf[0] : 0.; h[a + 5] = okg ? mg[a] / mg[0] : 0.; }
    h[5] = mf[0] + mg[0];
#pragma unroll
    for (int c = 0; c < BFLBM_NHYDROBAR; ++c) if (sel.mask & (1u << c)) o[(long long)sel.slot[c] * n] = h[c];
    return;
  }
  const double* __restrict__ rho = R->rho;
  const double* __restrict__ phi = R->phi;
  RefState Rf;
  Rf.rho = Rf.phi = Rf.rhot = nullptr;
  Rf.on = 0; Rf.sx = Rf.sy = Rf.sz = 0;
  double fn[Q], gn[Q];
  if (P.noise_on) {
    double ar, ap, at;
    noise_state(Rf, G, x, y, p, r, ph, ar, ap, at);
    d_noise(P, ar, ap, at, global_site(G, x, y, p), R->idx0 + (uint32_t)k, ntab, fn, gn);
  } else {
#pragma unroll
    for (int a = 0; a < Q; ++a) { fn[a] = 0.; gn[a] = 0.; }
  }
  double nb[Q], grad_rho[3], grad_phi[3];
  gather_field(rho, I, nb); d_gradient(P, nb, grad_rho);
  gather_field(phi, I, nb); d_gradient(P, nb, grad_phi);
  SiteHydro Hy;
  SiteRecip Rc;
  d_site_recips(P, r, ph, Rc);
  d_hydrovars(P, fs, gs, r, ph, grad_rho, grad_phi, fn, gn, Hy, Rc);
  double h[BFLBM_NHYDRO_];
  h[0] = r; h[1] = ph; h[5] = r + ph;
  const double rho_tot = r + ph;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    h[2+a] = Hy.uf[a]; h[6+a] = Hy.ug[a]; h[9+a] = Hy.af[a]; h[12+a] = Hy.ag[a];
    h[15+a] = d_div(r*Hy.ufbar[a] + ph*Hy.ugbar[a] + 0.5*(r*Hy.af[a] + ph*Hy.ag[a]), rho_tot, Rc.tot);
  }
  h[18] = Hy.nfvel[0]; h[19] = Hy.ngvel[0]; h[20] = Hy.ufbar[0]; h[21] = Hy.ugbar[0];
#pragma unroll
  for (int c = 0; c < BFLBM_NHYDRO_; ++c) if (sel.mask & (1u << c)) o[(long long)sel.slot[c] * n] = h[c];
}

// grid (ceil(nk / 256), npairs, B): acc[r][p][k] += scale[p] * a^(k) conj(b^(k)) / N, the arithmetic of k_sf_accumulate
__global__ void __launch_bounds__(256) k_sf_accumulate_batch(const double2* __restrict__ hat, double2* __restrict__ acc,
                                                             long long nk, int nsel, SfPairs P, double inv_n) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nk) return;
  const int p = blockIdx.y;
  const double2* __restrict__ mine = hat + (long long)blockIdx.z * nsel * nk;
  const double2 a = mine[(long long)P.a[p] * nk + k], b = mine[(long long)P.b[p] * nk + k];
  const double s = P.scale[p];
  const double ar = s * a.x, ai = s * a.y;
  const long long at = ((long long)blockIdx.z * P.n + p) * nk + k;
  double2 v = acc[at];
  v.x += (ar * b.x + ai * b.y) * inv_n;
  v.y += (ai * b.x - ar * b.y) * inv_n;
  acc[at] = v;
}

// grid (ceil(n / 256), npairs): the full fft-shifted mean spectrum as k_sf_expand forms it, of replica `replica`
// (inv = 1 / nsamples) or, replica < 0, of the ensemble: the nrep accumulators of the (pair, k) added in the order
// 0 ... nrep-1, times inv = 1 / (nrep nsamples).  what: 0 |S| (of the complex mean), 1 Re S, 2 Im S
__global__ void __launch_bounds__(256) k_sf_expand_batch(const double2* __restrict__ acc, double* __restrict__ out,
                                                         int nx, int ny, int nz, int npairs, int nrep, int replica,
                                                         double inv, int what, int zero_avg) {
  const long long n = (long long)nx * ny * nz;
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const int p = blockIdx.y;
  const int xs = (int)(s % nx), ys = (int)((s / nx) % ny), zs = (int)(s / ((long long)nx * ny));
  int kx = xs - nx / 2; if (kx < 0) kx += nx;
  int ky = ys - ny / 2; if (ky < 0) ky += ny;
  int kz = zs - nz / 2; if (kz < 0) kz += nz;
  const int nxc = nx / 2 + 1;
  const long long nk = (long long)nxc * ny * nz;
  const bool own = kx < nxc;                           // otherwise S(-k) = conj(S(k)) for real fields
  const int mx = own ? kx : nx - kx, my = own ? ky : (ny - ky) % ny, mz = own ? kz : (nz - kz) % nz;
  const long long at = (long long)p * nk + ((long long)mz * ny + my) * nxc + mx;
  double re, im;
  if (replica >= 0) {
    const double2 v = acc[(long long)replica * npairs * nk + at];
    re = v.x; im = v.y;
  } else {
    re = 0.; im = 0.;
    for (int r = 0; r < nrep; ++r) { const double2 v = acc[(long long)r * npairs * nk + at]; re += v.x; im += v.y; }
  }
  if (!own) im = -im;
  re *= inv; im *= inv;
  if (zero_avg && kx == 0 && ky == 0 && kz == 0) { re = 0.; im = 0.; }
  out[(long long)p * n + s] = (what == 0) ? hypot(re, im) : (what == 1 ? re : im);
}

// One observation launch over the whole batch into `out` ([B][sel.nsel][n]); what 0 hydrovsbar, 2 hydrovs.  hydrovs reads
// rho / phi: where some replica's are not those of its resident state, one k_density_batch launch rewrites them all.
int batch_observe_launch(bflbm_batch* b, int what, const ObsSel& sel, double* out, const char* call) {
  for (const bflbm_ctx* c : b->ctx) if (c->step_open()) return fail("%s: a replica has an open step", call);
  HIP_TRY(hipSetDevice(b->device));
  if (batch_sync_table(b)) return 1;                   // a frame between steps (k = 0 after an init or upload): stale records
  const Geo& G = b->G;
  const dim3 grid((unsigned)((G.plane + 255) / 256), (unsigned)G.nzs, (unsigned)b->ctx.size()), block(256);
  if (what == 2) {
    bool valid = true;
    for (const bflbm_ctx* c : b->ctx) valid = valid && c->density_valid;
    if (!valid) {
      hipLaunchKernelGGL(k_density_batch, grid, block, 0, b->stream, b->d_rec, G, (int)b->k);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return fail("%s: density launch failed: %s", call, hipGetErrorString(e));
      for (bflbm_ctx* c : b->ctx) density_computed(c);
    }
    hipLaunchKernelGGL((k_observe_batch<2>), grid, block, 0, b->stream, b->d_rec, out, G, (int)b->k, sel);
  } else {
    hipLaunchKernelGGL((k_observe_batch<0>), grid, block, 0, b->stream, b->d_rec, out, G, (int)b->k, sel);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("%s: observation launch failed: %s", call, hipGetErrorString(e));
  return 0;
}

}  // namespace

struct bflbm_batch_sf : bflbm_recorder {  // n: frames accumulated; every == 0: fed by bflbm_batch_sf_accumulate only
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0, nk = 0;     // sites, half-spectrum size
  SfPairs pairs;                    // a, b: slots of the pair's variables
  FieldSelection fs;                // the distinct variables of the pairs
  double* fields = nullptr;         // [nrep][nsel][nsites]
  double2* hat = nullptr;           // [nrep][nsel][nk]
  double2* acc = nullptr;           // [nrep][npairs][nk]
  double* expand = nullptr;         // [npairs][nsites]
  hipfftHandle plan = nullptr;
  size_t acc_bytes() const { return (size_t)nrep * pairs.n * nk * sizeof(double2); }
  bflbm_batch_sf() : bflbm_recorder("structure-factor accumulator", "bflbm_batch_sf") {}
  int record() override;
};

namespace {

// where the spectra of accepted pairs lie among the selection's, and their scales (null: 1.0)
SfPairs sf_pairs(const ObsSel& sel, int npairs, const int* var_a, const int* var_b, const double* scale) {
  SfPairs P;
  P.n = npairs;
  for (int p = 0; p < 32; ++p) {
    P.a[p] = p < npairs ? sel.slot[var_a[p]] : 0;
    P.b[p] = p < npairs ? sel.slot[var_b[p]] : 0;
    P.scale[p] = (p < npairs && scale) ? scale[p] : 1.0;
  }
  return P;
}

void batch_sf_free(bflbm_batch_sf* s) {
  if (s->plan) g_fft.destroy(s->plan);
  for (void* p : {(void*)s->fields, (void*)s->hat, (void*)s->acc, (void*)s->expand}) if (p) hipFree(p);
  delete s;
}

// enqueue one frame of the resident state of every replica; no host synchronisation
int batch_sf_frame(bflbm_batch_sf* s, const char* call) {
  bflbm_batch* b = s->batch;
  if (batch_observe_launch(b, field_observe_code(s->fs.source), s->fs.sel, s->fields, call)) return 1;
  g_fft.set_stream(s->plan, b->stream);
  if (g_fft.exec_d2z(s->plan, s->fields, (hipfftDoubleComplex*)s->hat) != HIPFFT_SUCCESS) return fail("%s: hipfftExecD2Z failed", call);
  const dim3 grid((unsigned)((s->nk + 255) / 256), (unsigned)s->pairs.n, (unsigned)s->nrep);
  hipLaunchKernelGGL(k_sf_accumulate_batch, grid, dim3(256), 0, b->stream, s->hat, s->acc, s->nk, s->fs.sel.nsel, s->pairs, 1.0 / (double)s->nsites);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("%s: accumulation launch failed: %s", call, hipGetErrorString(e));
  s->n += 1;
  return 0;
}

void batch_obs_free(bflbm_batch* b) {
  if (b->d_obs) hipFree(b->d_obs);
  b->d_obs = nullptr; b->obs_doubles = 0;
}

int batch_get(bflbm_batch* b, int what, int ncomp, double* dst, const char* call) {
  if (!b || !dst) return fail("%s: null argument", call);
  const int most = what == 2 ? BFLBM_NHYDRO : BFLBM_NHYDROBAR;
  if (ncomp < 1 || ncomp > most) return fail("%s: ncomp must be 1..%d (got %d)", call, most, ncomp);
  HIP_TRY(hipSetDevice(b->device));
  const size_t n = (size_t)b->G.nzs * (size_t)b->G.dplane;
  const size_t want = b->ctx.size() * (size_t)ncomp * n;
  if (b->obs_doubles < want) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    batch_obs_free(b);
    const hipError_t e = hipMalloc((void**)&b->d_obs, want * sizeof(double));
    if (e != hipSuccess) { (void)hipGetLastError(); b->d_obs = nullptr; return fail("%s: out of device memory (%zu bytes)", call, want * sizeof(double)); }
    b->obs_doubles = want;
  }
  if (batch_observe_launch(b, what, obs_first(ncomp), b->d_obs, call)) return 1;
  HIP_TRY(hipMemcpyAsync(dst, b->d_obs, want * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

}  // namespace

int bflbm_batch_sf::record() { return batch_sf_frame(this, "bflbm_batch_step (structure-factor frame)"); }

extern "C" {

int bflbm_batch_sf_create(bflbm_batch* b, int npairs, const int* var_a, const int* var_b, const double* scale,
                          int lb_hydrovars, int every, bflbm_batch_sf** out) {
  if (!b || !var_a || !var_b || !out) return fail("bflbm_batch_sf_create: null argument");
  if (npairs < 1 || npairs > 32) return fail("bflbm_batch_sf_create: 1..32 pairs (got %d)", npairs);
  if (every < 0) return fail("bflbm_batch_sf_create: every must be >= 0 (got %d)", every);
  if (field_refuse_pair_vars("bflbm_batch_sf_create", lb_hydrovars ? 1 : 0, npairs, var_a, var_b)) return 1;
  if (load_fft()) return 1;
  HIP_TRY(hipSetDevice(b->device));
  bflbm_batch_sf* s = new bflbm_batch_sf();
  recorder_bind(s, nullptr, b, every);
  s->nx = b->G.nx; s->ny = b->G.ny; s->nz = b->G.nzs;
  s->nsites = (long long)s->nx * s->ny * s->nz;
  s->nk = (long long)(s->nx / 2 + 1) * s->ny * s->nz;
  s->fs = field_select_pairs(lb_hydrovars ? 1 : 0, npairs, var_a, var_b);
  s->pairs = sf_pairs(s->fs.sel, npairs, var_a, var_b, scale);
  const int nsel = s->fs.sel.nsel;
  const size_t fb = (size_t)s->nrep * nsel * s->nsites * sizeof(double), hb = (size_t)s->nrep * nsel * s->nk * sizeof(double2);
  const size_t ab = s->acc_bytes(), eb = (size_t)npairs * s->nsites * sizeof(double);
  hipError_t e = hipMalloc((void**)&s->fields, fb);
  if (e == hipSuccess) e = hipMalloc((void**)&s->hat, hb);
  if (e == hipSuccess) e = hipMalloc((void**)&s->acc, ab);
  if (e == hipSuccess) e = hipMalloc((void**)&s->expand, eb);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    batch_sf_free(s);
    return fail("bflbm_batch_sf_create: out of device memory (fields %zu + spectra %zu + accumulators %zu + download %zu bytes): %s", fb, hb, ab, eb, hipGetErrorString(e));
  }
  int dims[3] = {s->nz, s->ny, s->nx};
  if (g_fft.plan_many(&s->plan, 3, dims, nullptr, 1, (int)s->nsites, nullptr, 1, (int)s->nk, HIPFFT_D2Z, s->nrep * nsel) != HIPFFT_SUCCESS) {
    s->plan = nullptr;
    batch_sf_free(s);
    return fail("bflbm_batch_sf_create: hipfftPlanMany failed for %d transforms of %d x %d x %d", (int)b->ctx.size() * nsel, b->G.nx, b->G.ny, b->G.nzs);
  }
  g_fft.set_stream(s->plan, b->stream);
  e = hipMemsetAsync(s->acc, 0, ab, b->stream);
  if (e != hipSuccess) { batch_sf_free(s); return fail("bflbm_batch_sf_create: %s", hipGetErrorString(e)); }
  b->recorders.push_back(s);
  *out = s;
  return 0;
}

int bflbm_batch_sf_destroy(bflbm_batch_sf* s) {
  if (!s) return 0;
  recorder_detach(s);                                  // waits for the frames in flight: they write the buffers freed below
  hipSetDevice(s->device);
  batch_sf_free(s);
  return 0;
}

int bflbm_batch_sf_reset(bflbm_batch_sf* s) {
  if (!s) return fail("bflbm_batch_sf_reset: null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_bytes(), s->batch ? s->batch->stream : nullptr));
  s->n = 0; s->since = 0;
  return 0;
}

int bflbm_batch_sf_accumulate(bflbm_batch_sf* s, int reset) {
  if (!s) return fail("bflbm_batch_sf_accumulate: null argument");
  if (!s->batch) return fail("bflbm_batch_sf_accumulate: the batch of the accumulator was destroyed");
  if (reset) {                                         // FortStructure's reset: a new average; the every-count does not move
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_bytes(), s->batch->stream));
    s->n = 0;
  }
  return batch_sf_frame(s, "bflbm_batch_sf_accumulate");
}

int bflbm_batch_sf_nsamples(const bflbm_batch_sf* s, long long* n) {
  if (!s || !n) return fail("bflbm_batch_sf_nsamples: null argument");
  *n = s->n;
  return 0;
}

int bflbm_batch_sf_get(bflbm_batch_sf* s, int replica, int what, int zero_avg, double* dst) {
  if (!s || !dst) return fail("bflbm_batch_sf_get: null argument");
  if (replica < -1 || replica >= s->nrep) return fail("bflbm_batch_sf_get: replica %d of a batch of %d (-1: the ensemble mean)", replica, s->nrep);
  if (what < 0 || what > 2) return fail("bflbm_batch_sf_get: what must be 0, 1 or 2");
  HIP_TRY(hipSetDevice(s->device));
  const hipStream_t stream = s->batch ? s->batch->stream : nullptr;   // detaching waited for everything enqueued
  const long long frames = std::max(s->n, 1LL);
  const double inv = 1.0 / (replica < 0 ? (double)s->nrep * (double)frames : (double)frames);
  const dim3 grid((unsigned)((s->nsites + 255) / 256), (unsigned)s->pairs.n);
  hipLaunchKernelGGL(k_sf_expand_batch, grid, dim3(256), 0, stream, s->acc, s->expand, s->nx, s->ny, s->nz, s->pairs.n, s->nrep,
                     replica, inv, what, zero_avg);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, s->expand, (size_t)s->pairs.n * s->nsites * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int bflbm_batch_get_hydrovs(bflbm_batch* b, double* dst, int ncomp) { return batch_get(b, 2, ncomp, dst, "bflbm_batch_get_hydrovs"); }
int bflbm_batch_get_hydrovsbar(bflbm_batch* b, double* dst, int ncomp) { return batch_get(b, 0, ncomp, dst, "bflbm_batch_get_hydrovsbar"); }

}  // extern "C"

#endif  // BFLBM_BATCH_SF_H_
