// bflbm_fieldsel.h -- the one field-selection layer of the recorders that read observed fields: field statistics
// (bflbm_fstat.h), profile, radial and mode traces (bflbm_profile.h, bflbm_radial.h, bflbm_modes.h) and, through the
// transform layer (bflbm_spectra.h), the structure factors and the spectrum traces.  A kind chooses
// variables of one source (hydrovs, hydrovsbar or the noise moments) and, some kinds, pairs of them.  Here is what the
// kinds share around their kernels: the refusals of those arguments, the selection that tells the observation what to
// write and the kernels where to read it, the observation itself, the choice of a kernel's NV instantiation and the
// refusal of an open step.  The types below are by-value kernel parameters: their names and layouts are the kernels'.
// Host part: plain C++17 that needs the BFLBM_NHYDRO* constants and a declared int fail(const char*, ...); a stand-alone
// program defines BFLBM_FIELDSEL_HOST_ONLY and includes it alone (tests/fieldsel_main.cpp).  HIP part: included by
// bflbm.hip after bflbm_recorder.h and before every kind (needs bflbm_ctx, bflbm_batch, bflbm_ring, observe_launch,
// ring_step_open; batch_observe_launch of bflbm_batch_sf.h is declared here).
#ifndef BFLBM_FIELDSEL_H_
#define BFLBM_FIELDSEL_H_

#include <algorithm>
#include <initializer_list>
#include <type_traits>

namespace fstat_limits {
constexpr int kMaxVars = 8, kMaxPairs = 16;
}

// where the variables lie among the dense volumes of the observation, and the pairs as variable slots; by value
struct FstatVars { int vol[fstat_limits::kMaxVars]; };
struct FstatPairs { int n; int a[fstat_limits::kMaxPairs]; int b[fstat_limits::kMaxPairs]; };

namespace {

// which components an observation writes and where: component c with bit c of mask set goes to slot[c] of the replica's
// nsel dense volumes
struct ObsSel { unsigned mask; int nsel; int slot[BFLBM_NHYDRO_]; };

ObsSel obs_first(int ncomp) {
  ObsSel s; s.mask = 0; s.nsel = ncomp;
  for (int c = 0; c < BFLBM_NHYDRO_; ++c) { s.slot[c] = c < ncomp ? c : 0; if (c < ncomp) s.mask |= 1u << c; }
  return s;
}

// what a kind keeps of its chosen variables
struct FieldSelection {
  int source = 0;                   // 0 hydrovs, 1 hydrovsbar, 2 the noise moments
  int nvars = 0;
  int ncomp = 0;                    // a context: the components its observation produces
  ObsSel sel;                       // a batch: what the observation writes
  FstatVars vol;                    // the volume of the first kMaxVars variables: a batch's slot, a context's component
};

constexpr int kFieldNoiseMoments = 2 * 19;   // fa0 .. fa18, ga0 .. ga18

int field_source_size(int source) { return source == 0 ? BFLBM_NHYDRO : (source == 1 ? BFLBM_NHYDROBAR : kFieldNoiseMoments); }
const char* field_source_name(int source) { return source == 0 ? "hydrovs" : (source == 1 ? "hydrovsbar" : "the noise moments"); }
// observe_launch's and batch_observe_launch's code of a source: 2 hydrovs, 0 hydrovsbar, 1 noise
int field_observe_code(int source) { return source == 0 ? 2 : (source == 1 ? 0 : 1); }

// What every creation call refuses about its source, its variables and its pairs of variable slots.  max_source: the
// largest source the kind takes; a kind with a lb_hydrovars flag passes the flag as 0 or 1 and max_source 1, a kind
// without pairs npairs 0.
int field_refuse_args(const char* call, int source, int max_source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b) {
  using namespace fstat_limits;
  if (source < 0 || source > max_source)
    return max_source == 2 ? fail("%s: source must be 0 (hydrovs), 1 (hydrovsbar) or 2 (noise) (got %d)", call, source)
                           : fail("%s: source must be 0 (hydrovs) or 1 (hydrovsbar) (got %d)", call, source);
  if (nvars < 1 || nvars > kMaxVars) return fail("%s: 1..%d variables (got %d)", call, kMaxVars, nvars);
  if (npairs < 0 || npairs > kMaxPairs) return fail("%s: 0..%d pairs (got %d)", call, kMaxPairs, npairs);
  if (npairs > 0 && (!pair_a || !pair_b)) return fail("%s: null argument", call);
  const int most = field_source_size(source);
  for (int i = 0; i < nvars; ++i) {
    if (vars[i] < 0 || vars[i] >= most) return fail("%s: variable index %d outside %s (0..%d)", call, vars[i], field_source_name(source), most - 1);
    for (int k = 0; k < i; ++k) if (vars[k] == vars[i]) return fail("%s: variable index %d given twice", call, vars[i]);
  }
  for (int p = 0; p < npairs; ++p)
    for (int slot : {pair_a[p], pair_b[p]})
      if (slot < 0 || slot >= nvars) return fail("%s: pair %d: slot %d outside the %d variables", call, p, slot, nvars);
  return 0;
}

// the same for the kinds that take pairs of components (the spectra)
int field_refuse_pair_vars(const char* call, int source, int npairs, const int* var_a, const int* var_b) {
  const int most = field_source_size(source);
  for (int p = 0; p < npairs; ++p)
    for (int v : {var_a[p], var_b[p]})
      if (v < 0 || v >= most) return fail("%s: pair %d: variable index %d outside %s (0..%d)", call, p, v, field_source_name(source), most - 1);
  return 0;
}

// The selection of accepted variables.  The batch observation writes the chosen variables in ascending order (a batch has
// no noise form, so a bit of the mask is a hydrovs component); a context's observation all components up to the largest.
FieldSelection field_select(bool batch, int source, int nvars, const int* vars) {
  FieldSelection f;
  f.source = source; f.nvars = nvars;
  f.sel.mask = 0; f.sel.nsel = 0;
  int top = 0;
  for (int i = 0; i < nvars; ++i) { if (batch) f.sel.mask |= 1u << vars[i]; top = std::max(top, vars[i]); }
  for (int v = 0; v < BFLBM_NHYDRO_; ++v) f.sel.slot[v] = (f.sel.mask & (1u << v)) ? f.sel.nsel++ : 0;
  f.ncomp = source == 0 ? top + 1 : field_source_size(source);
  for (int i = 0; i < fstat_limits::kMaxVars; ++i) f.vol.vol[i] = i < nvars ? (batch ? f.sel.slot[vars[i]] : vars[i]) : 0;
  return f;
}

// The selection of the distinct components of accepted pairs, ascending (nvars of them, up to BFLBM_NHYDRO_).  A spectrum
// lies at sel.slot[component] of a replica for a context too: the mask is filled either way.
FieldSelection field_select_pairs(int source, int npairs, const int* var_a, const int* var_b) {
  bool chosen[BFLBM_NHYDRO_] = {};
  for (int p = 0; p < npairs; ++p) { chosen[var_a[p]] = true; chosen[var_b[p]] = true; }
  int vars[BFLBM_NHYDRO_], n = 0;
  for (int v = 0; v < BFLBM_NHYDRO_; ++v) if (chosen[v]) vars[n++] = v;
  return field_select(true, source, n, vars);
}

FstatPairs field_pairs(int npairs, const int* pair_a, const int* pair_b) {
  FstatPairs P;
  P.n = npairs;
  for (int p = 0; p < fstat_limits::kMaxPairs; ++p) { P.a[p] = p < npairs ? pair_a[p] : 0; P.b[p] = p < npairs ? pair_b[p] : 0; }
  return P;
}

}  // namespace

#ifndef BFLBM_FIELDSEL_HOST_ONLY

namespace {

static_assert(kFieldNoiseMoments == 2 * Q, "the noise moments of both fluids");

int batch_observe_launch(bflbm_batch* b, int what, const ObsSel& sel, double* out, const char* call);   // bflbm_batch_sf.h

// A creation call inside an open step.  Only bflbm_step_boundary opens a step and it refuses a replica of a batch, so
// the replica form never fires today; every kind takes the full check all the same.
int recorder_refuse_open(const bflbm_ctx* c, const bflbm_batch* b, const bflbm_ring* g, const char* call) {
  if ((c && c->step_open()) || (g && ring_step_open(g))) return fail("%s inside an open step", call);
  if (b) for (const bflbm_ctx* v : b->ctx) if (v->step_open()) return fail("%s: a replica has an open step", call);
  return 0;
}

// Observe the selection of one context (a lone one or a slab of a ring) into its scratch state buffer: *dense is
// [comp][z][y][x] over the own planes, as bflbm_sf_accumulate reads it.  Selects the context's device.
int fields_observe_slab(bflbm_ctx* c, const FieldSelection& f, const char* asker, const double** dense) {
  if (observe_launch(c, field_observe_code(f.source), f.ncomp, asker)) return 1;
  *dense = c->S[1 - c->cur];
  return 0;
}

// Observe the selection of the recorder's lone context or batch: variable i of replica r then lies at
// *dense + r * *rep_stride + f.vol.vol[i] * sites.  A batch observes into batch_fields, [nrep][sel.nsel][sites].
int fields_observe(const bflbm_recorder* rec, const FieldSelection& f, double* batch_fields, const char* asker,
                   const double** dense, long long* rep_stride) {
  *rep_stride = 0;
  if (!rec->batch) return fields_observe_slab(rec->ctx, f, asker, dense);
  if (batch_observe_launch(rec->batch, field_observe_code(f.source), f.sel, batch_fields, asker)) return 1;
  *dense = batch_fields;
  *rep_stride = (long long)f.sel.nsel * rec->batch->G.nzs * rec->batch->G.dplane;
  return 0;
}

// launch(std::integral_constant<int, NV>()) for NV == nvars in 1 .. kMaxVars: how a kind picks the instantiation of a
// kernel whose variable count is a template parameter.  false: nvars is outside, nothing was called.
template <int NV = 1, class Launch> bool field_dispatch_nv(int nvars, Launch&& launch) {
  if constexpr (NV > fstat_limits::kMaxVars) return false;
  else {
    if (nvars == NV) { launch(std::integral_constant<int, NV>()); return true; }
    return field_dispatch_nv<NV + 1>(nvars, launch);
  }
}

}  // namespace

#endif  // BFLBM_FIELDSEL_HOST_ONLY

#endif  // BFLBM_FIELDSEL_H_
