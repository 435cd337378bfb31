// bflbm_sf_ring.h -- structure factors of a lattice that is decomposed into z-slabs (bflbm_ring), needed by
// configs[4]-style multi-GPU runs whose primary fluctuation check is FHDeX's StructFact on hydrovs
// (main_run_job.cpp:301-310, :342-349).  Same definition and normalisation as bflbm_sf.h.  One frame: the slab transform
// of bflbm_spectra.h, then k_sf_accumulate on every slab's rows into the slab's own acc[pair][kz][ky local][kx'],
// stream-ordered like a sample of the ring's spectrum trace.  bflbm_ring_sf_get assembles the half spectrum on the
// host and expands it with sf_site / sf_value, as k_sf_expand does.  A ring of one slab delegates to bflbm_sf of ctx[0].
// The link to the ring and the detaching are those of bflbm_recorder.h, as for bflbm_sf.
#ifndef BFLBM_SF_RING_H_
#define BFLBM_SF_RING_H_

struct bflbm_ring_sf : bflbm_recorder {
  bflbm_sf* single = nullptr;       // a ring of one slab: the lone accumulator of ctx[0]; the rest stays empty, unbound
  int nx = 0, ny = 0, nz = 0;
  SpectraSelection sel;             // selected against hydrovs
  SlabSpectra T;
  std::vector<double2*> acc;        // per slab, on its device: [pair][nz][nky][nxc]
  size_t acc_bytes(size_t k) const { return (size_t)sel.pairs.n * T.slab[k].nk * sizeof(double2); }
  hipStream_t stream(size_t k) const { return ring ? ring->ctx[k]->stream : nullptr; }   // detaching waited for everything enqueued
  bflbm_ring_sf() : bflbm_recorder("structure-factor accumulator", "bflbm_ring_sf") {}
  ~bflbm_ring_sf() override {
    if (single) bflbm_sf_destroy(single);
    for (size_t k = 0; k < acc.size(); ++k) if (acc[k]) { hipSetDevice(T.slab[k].device); hipFree(acc[k]); }
  }
  int record() override;
};

namespace {

int ring_sf_reset(bflbm_ring_sf* s) {
  s->n = 0;
  for (size_t k = 0; k < s->acc.size(); ++k) {
    HIP_TRY(hipSetDevice(s->T.slab[k].device));
    HIP_TRY(hipMemsetAsync(s->acc[k], 0, s->acc_bytes(k), s->stream(k)));
  }
  return 0;
}

int ring_sf_accumulate(const char* call, bflbm_ring_sf* s, int lb_hydrovars, int reset) {
  if (s->single) return sf_accumulate(call, s->single, lb_hydrovars, reset);
  if (!recorder_attached(s)) return fail("%s: the ring of the accumulator was destroyed", call);
  if (recorder_owner_open(s)) return fail("%s inside an open step", call);
  FieldSelection frame;
  if (sf_frame_selection(call, s->sel.fs, lb_hydrovars, &frame)) return 1;
  if (reset && ring_sf_reset(s)) return 1;
  const double inv_n = 1.0 / ((double)s->nx * s->ny * s->nz);
  if (slab_run(s->T, s->ring, frame, s->sel.vars, call, [&](int d, const double2* zb, long long nk, hipStream_t stream) {
        return sf_accumulate_launch(zb, s->acc[(size_t)d], nk, s->sel.nspec, s->sel.pairs, 1, inv_n, stream);
      })) return 1;
  s->n += 1;
  return 0;
}

}  // namespace

int bflbm_ring_sf::record() { return ring_sf_accumulate("bflbm_ring_sf (frame)", this, 0, 0); }

extern "C" {

int bflbm_ring_sf_destroy(bflbm_ring_sf* s) {
  if (!s) return 0;
  recorder_detach(s);                                  // waits for the frames in flight on every slab's stream
  delete s;
  return 0;
}

int bflbm_ring_sf_create(bflbm_ring* r, int npairs, const int* var_a, const int* var_b, const double* scale, bflbm_ring_sf** out) {
  const char* call = "bflbm_ring_sf_create";
  if (!r || !var_a || !var_b || !out) return fail("%s: null argument", call);
  std::unique_ptr<bflbm_ring_sf> s(new bflbm_ring_sf());
  if (r->ctx.size() == 1) {
    if (sf_create(call, r->ctx[0], npairs, var_a, var_b, scale, &s->single)) return 1;
    *out = s.release();
    return 0;
  }
  if (sf_refuse_args(call, npairs, var_a, var_b)) return 1;
  if (recorder_refuse_open(nullptr, nullptr, r, call)) return 1;
  if (load_fft()) return 1;
  recorder_bind(s.get(), nullptr, nullptr, 0, r);
  const Geo& G = r->ctx[0]->G;
  s->nx = G.nx; s->ny = G.ny; s->nz = G.nz;
  s->sel = spectra_select(0, npairs, var_a, var_b, scale);
  if (slab_create(s->T, call, r, s->sel.nspec)) return 1;
  s->acc.assign(r->ctx.size(), nullptr);
  for (size_t k = 0; k < s->acc.size(); ++k) {
    hipError_t e = hipSetDevice(s->T.slab[k].device);
    if (e == hipSuccess) e = hipMalloc((void**)&s->acc[k], s->acc_bytes(k));
    if (e == hipSuccess) e = hipMemsetAsync(s->acc[k], 0, s->acc_bytes(k), r->ctx[k]->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail("%s: accumulators of slab %zu (%zu bytes): %s", call, k, s->acc_bytes(k), hipGetErrorString(e)); }
  }
  r->recorders.push_back(s.get());
  *out = s.release();
  return 0;
}

int bflbm_ring_sf_reset(bflbm_ring_sf* s) {
  if (!s) return fail("bflbm_ring_sf_reset: null argument");
  return s->single ? sf_reset(s->single) : ring_sf_reset(s);
}

int bflbm_ring_sf_nsamples(const bflbm_ring_sf* s, long long* n) {
  if (!s || !n) return fail("bflbm_ring_sf_nsamples: null argument");
  *n = s->single ? s->single->n : s->n;
  return 0;
}

int bflbm_ring_sf_accumulate(bflbm_ring_sf* s, int lb_hydrovars, int reset) {
  if (!s) return fail("bflbm_ring_sf_accumulate: null argument");
  return ring_sf_accumulate("bflbm_ring_sf_accumulate", s, lb_hydrovars, reset);
}

// mean over the accumulated frames, fft-shifted, dst[npairs][nz][ny][nx] on the host (like bflbm_sf_get); reads only
// what the handle owns, so it serves a detached accumulator too
int bflbm_ring_sf_get(bflbm_ring_sf* s, int what, int zero_avg, double* dst) {
  const char* call = "bflbm_ring_sf_get";
  if (!s || !dst) return fail("%s: null argument", call);
  if (s->single) return sf_get(call, s->single, what, zero_avg, dst);
  if (what < 0 || what > 2) return fail("%s: what must be 0, 1 or 2", call);
  const int nx = s->nx, ny = s->ny, nz = s->nz, nxc = s->T.nxc, np = s->sel.pairs.n;
  // half spectrum acc[pair][kz][ky][kx'] assembled from the slabs' row blocks
  const size_t nk = (size_t)nz * ny * nxc;
  std::vector<double2> acc((size_t)np * nk);
  for (size_t k = 0; k < s->acc.size(); ++k) {
    const SlabSpectra::Slab& q = s->T.slab[k];
    const size_t row = (size_t)(q.ky1 - q.ky0) * nxc * sizeof(double2);
    HIP_TRY(hipSetDevice(q.device));
    HIP_TRY(hipStreamSynchronize(s->stream(k)));
    // [pair][kz] blocks of nky*nxc contiguous -> rows ky0.. of the full plane
    HIP_TRY(hipMemcpy2D(acc.data() + (size_t)q.ky0 * nxc, (size_t)ny * nxc * sizeof(double2), s->acc[k], row, row, (size_t)np * nz, hipMemcpyDeviceToHost));
  }
  const double inv_samples = 1.0 / (double)std::max(s->n, 1LL);
  const long long nn = (long long)nx * ny * nz;
  for (int p = 0; p < np; ++p)
    for (long long site = 0; site < nn; ++site) {
      const SfSite K = sf_site(site, nx, ny, nz);
      const double2 v = acc[(size_t)p * nk + (size_t)K.at];
      dst[(size_t)p * nn + site] = sf_value(v.x, v.y, K, inv_samples, what, zero_avg);
    }
  return 0;
}

}  // extern "C"

#endif  // BFLBM_SF_RING_H_
