// bflbm_sf.h -- running structure factors <a^(k) b^*(k)>/N of pairs of hydrodynamic fields on the GPU
// (SURVEY 8f rank 2).  The reference accumulates them with FHDeX's StructFact::FortStructure every
// out_SF_step steps (main_run_job.cpp:301-310, :342-349) and writes them with WritePlotFile (:50-54);
// FHDeX is un-vendored, so the definition follows the call sites and what Mixture.ipynb reads (see
// structfact.py, the host-side twin this is tested against).
// One frame of a lone context: the dense transform of bflbm_spectra.h of hydrovs (or hydrovsbar, chosen per frame),
// then k_sf_accumulate; bflbm_sf_get expands the mean over the frames into the context's scratch buffer.
// The link to the context and the detaching are those of bflbm_recorder.h: every == 0, stepping never serves the
// accumulator, n counts the frames.  record() takes a hydrovs frame.
#ifndef BFLBM_SF_H_
#define BFLBM_SF_H_

struct bflbm_sf : bflbm_recorder {
  int nx = 0, ny = 0, nz = 0;
  SpectraSelection sel;             // selected against hydrovs
  DenseSpectra T;
  double2* acc = nullptr;           // [npairs][nk]
  size_t acc_bytes() const { return (size_t)sel.pairs.n * T.nk * sizeof(double2); }
  bflbm_sf() : bflbm_recorder("structure-factor accumulator", "bflbm_sf") {}
  ~bflbm_sf() override { if (acc) { hipSetDevice(device); hipFree(acc); } }
  int record() override;
};

namespace {

// what the lone and the ring accumulator refuse about their pairs; they select against hydrovs
int sf_refuse_args(const char* call, int npairs, const int* var_a, const int* var_b) {
  if (npairs < 1 || npairs > 32) return fail("%s: 1..32 pairs (got %d)", call, npairs);
  return field_refuse_pair_vars(call, 0, npairs, var_a, var_b);
}
// the selection of one frame: hydrovs as selected, or all of hydrovsbar
int sf_frame_selection(const char* call, const FieldSelection& fs, int lb_hydrovars, FieldSelection* frame) {
  if (lb_hydrovars && fs.ncomp > BFLBM_NHYDROBAR) return fail("%s: pair variables outside hydrovsbar", call);
  *frame = fs;
  if (lb_hydrovars) { frame->source = 1; frame->ncomp = BFLBM_NHYDROBAR; }
  return 0;
}

// the calls of a lone accumulator; `call`: the C-ABI call that asks (a ring of one slab delegates here)
int sf_create(const char* call, bflbm_ctx* c, int npairs, const int* var_a, const int* var_b, const double* scale, bflbm_sf** out) {
  if (sf_refuse_args(call, npairs, var_a, var_b)) return 1;
  if (!c->G.zwrap) return fail("%s: structure factors need the whole lattice in one context (nranks == 1)", call);
  if (recorder_refuse_open(c, nullptr, nullptr, call)) return 1;
  if (load_fft()) return 1;
  std::unique_ptr<bflbm_sf> s(new bflbm_sf());
  recorder_bind(s.get(), c, nullptr, 0);
  s->nx = c->G.nx; s->ny = c->G.ny; s->nz = c->G.nz;
  s->sel = spectra_select(0, npairs, var_a, var_b, scale);
  if (dense_create(s->T, call, c, nullptr, s->sel.nspec)) return 1;
  if (hipMalloc((void**)&s->acc, s->acc_bytes()) != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: out of device memory (accumulators %zu bytes)", call, s->acc_bytes());
  }
  HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_bytes(), c->stream));
  c->recorders.push_back(s.get());
  *out = s.release();
  return 0;
}

int sf_reset(bflbm_sf* s) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemsetAsync(s->acc, 0, s->acc_bytes(), sf_stream(s)));
  s->n = 0;
  return 0;
}

// FortStructure(fields, reset): one frame of the resident state.  lb_hydrovars != 0 takes hydrovsbar
// (the shipped STRUCT_LB_HYDROVARS build, main_run_job.cpp:19, :344) instead of hydrovs.
int sf_accumulate(const char* call, bflbm_sf* s, int lb_hydrovars, int reset) {
  if (!recorder_attached(s)) return fail("%s: the context of the accumulator was destroyed", call);
  if (recorder_owner_open(s)) return fail("%s inside an open step", call);
  FieldSelection frame;
  if (sf_frame_selection(call, s->sel.fs, lb_hydrovars, &frame)) return 1;
  if (reset && sf_reset(s)) return 1;
  if (dense_run(s->T, s, frame, s->sel.vars, call)) return 1;
  if (sf_accumulate_launch(s->T.hat, s->acc, s->T.nk, s->sel.nspec, s->sel.pairs, 1, 1.0 / (double)s->T.nsites, s->ctx->stream)) return 1;
  s->n += 1;
  return 0;
}

// mean over the accumulated frames, fft-shifted (k = 0 at cell n/2), dst[npairs][nz][ny][nx] on the host;
// what: 0 magnitude, 1 real part, 2 imaginary part; zero_avg != 0 removes the k = 0 mode (WritePlotFile's flag)
int sf_get(const char* call, bflbm_sf* s, int what, int zero_avg, double* dst) {
  if (what < 0 || what > 2) return fail("%s: what must be 0, 1 or 2", call);
  if (!recorder_attached(s))
    return fail("%s: the context of the accumulator was destroyed, and the expansion is written into the context's scratch buffer", call);
  bflbm_ctx* c = s->ctx;
  if (c->step_open()) return fail("%s inside an open step", call);
  HIP_TRY(hipSetDevice(s->device));
  double* out = c->S[1 - c->cur];                      // 38 component volumes of scratch >= 32 pairs
  return sf_expand_get(s->acc, out, dst, s->nx, s->ny, s->nz, s->sel.pairs.n, 1, 0, s->n, what, zero_avg, c->stream);
}

}  // namespace

int bflbm_sf::record() { return sf_accumulate("bflbm_sf (frame)", this, 0, 0); }

extern "C" {

int bflbm_sf_create(bflbm_ctx* c, int npairs, const int* var_a, const int* var_b, const double* scale, bflbm_sf** out) {
  if (!c || !var_a || !var_b || !out) return fail("bflbm_sf_create: null argument");
  return sf_create("bflbm_sf_create", c, npairs, var_a, var_b, scale, out);
}
int bflbm_sf_destroy(bflbm_sf* s) {
  if (!s) return 0;
  recorder_detach(s);                                  // waits for the frames in flight: they write the buffers freed below
  delete s;
  return 0;
}
int bflbm_sf_reset(bflbm_sf* s) {
  if (!s) return fail("bflbm_sf_reset: null argument");
  return sf_reset(s);
}
int bflbm_sf_accumulate(bflbm_sf* s, int lb_hydrovars, int reset) {
  if (!s) return fail("bflbm_sf_accumulate: null argument");
  return sf_accumulate("bflbm_sf_accumulate", s, lb_hydrovars, reset);
}
int bflbm_sf_nsamples(const bflbm_sf* s, long long* n) {
  if (!s || !n) return fail("bflbm_sf_nsamples: null argument");
  *n = s->n;
  return 0;
}
int bflbm_sf_get(bflbm_sf* s, int what, int zero_avg, double* dst) {
  if (!s || !dst) return fail("bflbm_sf_get: null argument");
  return sf_get("bflbm_sf_get", s, what, zero_avg, dst);
}

}  // extern "C"

#endif  // BFLBM_SF_H_
