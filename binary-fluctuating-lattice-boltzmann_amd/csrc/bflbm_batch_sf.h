// bflbm_batch_sf.h -- ensemble structure factors: S(k) of every replica of a batch in one batched pass
// (include/bflbm.h, "Ensemble structure factors").  One accumulator per bflbm_sf costs a batch of B replicas B observation
// launches, B x (distinct variables) transforms and B accumulation launches per frame; here a frame is, on the batch's
// stream and without a host synchronisation, the dense transform of bflbm_spectra.h (k_observe_batch of the selected
// components of all replicas, one batched D2Z) and one k_sf_accumulate launch into the accumulators [B][npairs][nk].
// The accumulator owns its buffers; of the replicas only rho / phi are written, by one k_density_batch launch, when
// hydrovs is observed and some replica's densities are not those of its resident state.
// k_observe_batch computes, per site, what k_observe computes (the same device functions in the same order, no injected
// noise, no reference state), so the stacked getters bflbm_batch_get_hydrovs / _hydrovsbar return the doubles of the views'.
// The link to the batch, the every-count and the detaching are those of bflbm_recorder.h.
// Included by bflbm.hip after bflbm_batch.h, bflbm_spectra.h and bflbm_trace.h (needs bflbm_batch, ObsSel).
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
  SpectraSelection sel;             // of the source chosen at creation
  DenseSpectra T;                   // fields [nrep][nsel][nsites], hat [nrep][nsel][nk]
  double2* acc = nullptr;           // [nrep][npairs][nk]
  double* expand = nullptr;         // [npairs][nsites]
  size_t acc_bytes() const { return (size_t)nrep * sel.pairs.n * T.nk * sizeof(double2); }
  bflbm_batch_sf() : bflbm_recorder("structure-factor accumulator", "bflbm_batch_sf") {}
  ~bflbm_batch_sf() override {
    if (!acc && !expand) return;
    hipSetDevice(device);
    if (acc) hipFree(acc);
    if (expand) hipFree(expand);
  }
  int record() override;
};

namespace {

// enqueue one frame of the resident state of every replica; no host synchronisation
int batch_sf_frame(bflbm_batch_sf* s, const char* call) {
  if (dense_run(s->T, s, s->sel.fs, s->sel.vars, call)) return 1;
  if (sf_accumulate_launch(s->T.hat, s->acc, s->T.nk, s->sel.nspec, s->sel.pairs, s->nrep, 1.0 / (double)s->T.nsites, s->batch->stream)) return 1;
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
  std::unique_ptr<bflbm_batch_sf> s(new bflbm_batch_sf());
  recorder_bind(s.get(), nullptr, b, every);
  s->nx = b->G.nx; s->ny = b->G.ny; s->nz = b->G.nz;
  s->sel = spectra_select(lb_hydrovars ? 1 : 0, npairs, var_a, var_b, scale);
  if (dense_create(s->T, "bflbm_batch_sf_create", nullptr, b, s->sel.nspec)) return 1;
  const size_t ab = s->acc_bytes(), eb = (size_t)npairs * s->T.nsites * sizeof(double);
  hipError_t e = hipMalloc((void**)&s->acc, ab);
  if (e == hipSuccess) e = hipMalloc((void**)&s->expand, eb);
  if (e == hipSuccess) e = hipMemsetAsync(s->acc, 0, ab, b->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("bflbm_batch_sf_create: out of device memory (accumulators %zu + download %zu bytes): %s", ab, eb, hipGetErrorString(e));
  }
  b->recorders.push_back(s.get());
  *out = s.release();
  return 0;
}

int bflbm_batch_sf_destroy(bflbm_batch_sf* s) {
  if (!s) return 0;
  recorder_detach(s);                                  // waits for the frames in flight: they write the buffers freed below
  delete s;
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
  return sf_expand_get(s->acc, s->expand, dst, s->nx, s->ny, s->nz, s->sel.pairs.n, s->nrep, replica, s->n, what, zero_avg, sf_stream(s));
}

int bflbm_batch_get_hydrovs(bflbm_batch* b, double* dst, int ncomp) { return batch_get(b, 2, ncomp, dst, "bflbm_batch_get_hydrovs"); }
int bflbm_batch_get_hydrovsbar(bflbm_batch* b, double* dst, int ncomp) { return batch_get(b, 0, ncomp, dst, "bflbm_batch_get_hydrovsbar"); }

}  // extern "C"

#endif  // BFLBM_BATCH_SF_H_
