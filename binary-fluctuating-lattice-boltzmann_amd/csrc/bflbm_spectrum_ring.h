// bflbm_spectrum_ring.h -- the spectrum trace of a ring of z-slabs (include/bflbm.h, "Spectrum traces"): bins, weights
// and normalisation are those of bflbm_spectrum.h, the transform is the slab transform of bflbm_spectra.h.  A sample is,
// without a host synchronisation,
//   on every slab's stream      the slab transform, then k_spectrum_bin and k_spectrum_finish as they are with the slab's
//                               own tables (spectrum_tables::build_slab) into the slab's sums [pair][bin];
//   on slab 0's stream          the ring gather of bflbm_recorder.h: the slabs' sums into d_stage[slab][pair][bin], then
//                               k_spectrum_combine adds the slabs in the order 0 ... n-1 into the slot.
// A slab's sums wait for the gather's `taken` before the next sample overwrites them.  A record depends on the spectra,
// the slabs' tables and the slab count alone.  No atomics, no LDS beyond the tree of k_spectrum_bin, no scratch.
// Included by bflbm.hip after bflbm_spectrum.h (needs bflbm_ring).
#ifndef BFLBM_SPECTRUM_RING_H_
#define BFLBM_SPECTRUM_RING_H_

namespace {

// grid (ceil(nbins / 256), pairs): one thread per (bin, pair) adds the slabs' sums in slab order into the slot
__global__ void __launch_bounds__(256) k_spectrum_combine(const double* __restrict__ sums, double* __restrict__ out, int nbins, int nslabs) {
  const int bin = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (bin >= nbins) return;
  const long long at = (long long)blockIdx.y * nbins + bin, per_slab = (long long)gridDim.y * nbins;
  double acc = 0.;
  for (int d = 0; d < nslabs; ++d) acc += sums[d * per_slab + at];
  out[at] = acc;
}

int spectrum_ring_create(bflbm_ring* g, int npairs, const int* var_a, const int* var_b, const double* scale,
                         int lb_hydrovars, int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out) {
  const char* call = "bflbm_ring_spectrum_create";
  const int n = (int)g->ctx.size();
  const Geo& G = g->ctx[0]->G;
  uint64_t L = 0;
  if (spectrum_refuse_args(call, npairs, var_a, var_b, lb_hydrovars, kind, every, capacity)) return 1;
  if (recorder_refuse_open(nullptr, nullptr, g, call)) return 1;
  if (spectrum_refuse_box(call, kind, G, &L)) return 1;
  if (load_fft()) return 1;

  std::unique_ptr<bflbm_spectrum> t(new bflbm_spectrum());
  {                                                        // bins, count and q are the whole box's: a lone trace's
    spectrum_tables::Tables T;
    spectrum_tables::build(G.nx, G.ny, G.nz, kind, zero_avg, L, spectrum_tables::kChunkLen, T);
    spectrum_select(t.get(), G, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, T);
  }
  if (slab_create(t->slabs, call, g, t->sel.nspec)) return 1;
  const size_t per = (size_t)npairs * (size_t)t->nbins, sb = per * sizeof(double);   // a slab's bin sums: its block of the gather
  t->tab.resize((size_t)n);
  for (int d = 0; d < n; ++d) {
    const SlabSpectra::Slab& q = t->slabs.slab[d];
    spectrum_tables::Tables T;
    spectrum_tables::build_slab(G.nx, G.ny, G.nz, q.ky0, q.ky1, kind, zero_avg, L, spectrum_tables::kChunkLen, T);
    t->nchunks += (long long)T.chunks.size(); t->max_chunks_per_bin = std::max(t->max_chunks_per_bin, T.max_chunks_per_bin);
    if (spectrum_tables_upload(t->tab[d], call, q.device, T, npairs)) return 1;
  }
  HIP_TRY(gather_create(t->gather, g, [&](int) { return sb; }, [&](int d) { return (size_t)d * sb; }));
  const std::string shape = " x " + std::to_string(npairs) + " pairs x " + std::to_string(t->nbins) + " bins";
  if (store_attach(t.get(), nullptr, nullptr, call, every, capacity, per, (size_t)n * per, shape.c_str(), g)) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

int bflbm_spectrum::record_ring() {
  if (store_begin(this)) return 1;
  bflbm_ring* g = ring;
  const int n = (int)g->ctx.size();
  const SfPairs& pairs = sel.pairs;
  const double inv_n = 1.0 / (double)nsites;
  // the binning of every slab's own rows
  if (slab_run(slabs, g, sel.fs, sel.vars, "spectrum trace sample", [&](int d, const double2* zb, long long nk, hipStream_t stream) {
        const SpectrumTables& q = tab[(size_t)d];
        if (q.nchunks > 0) {
          hipLaunchKernelGGL(k_spectrum_bin, dim3((unsigned)q.nchunks, (unsigned)pairs.n, 1), dim3(256), 0, stream,
                             zb, q.d_list, q.d_chunks, q.partial, nk, sel.nspec, nx, pairs, inv_n);
          HIP_TRY(hipGetLastError());
        }
        if (gather_hold(gather, d, stream)) return 1;
        hipLaunchKernelGGL(k_spectrum_finish, dim3((unsigned)((nbins + 255) / 256), (unsigned)pairs.n, 1), dim3(256), 0, stream,
                           q.partial, q.d_bin_first, gather_target(gather, d, d_stage), nbins, std::max(q.nchunks, 1LL));
        HIP_TRY(hipGetLastError());
        return gather_ready(gather, d, stream);
      })) return 1;
  // slab 0 takes the sums and adds them in slab order
  HIP_TRY(hipSetDevice(device));
  const hipStream_t s0 = g->ctx[0]->stream;
  if (gather_take(gather, d_stage, s0)) return 1;
  hipLaunchKernelGGL(k_spectrum_combine, dim3((unsigned)((nbins + 255) / 256), (unsigned)pairs.n), dim3(256), 0, s0,
                     d_stage, store_slot(this), nbins, n);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_ring_spectrum_create(bflbm_ring* r, int npairs, const int* var_a, const int* var_b, const double* scale, int lb_hydrovars,
                               int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out) {
  if (!r || !var_a || !var_b || !out) return fail("bflbm_ring_spectrum_create: null argument");
  if (r->ctx.size() == 1)                                  // the whole box: the lone trace of ctx[0], served by its steps
    return bflbm_spectrum_create(r->ctx[0], npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, every, capacity, out);
  return spectrum_ring_create(r, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, every, capacity, out);
}

}  // extern "C"

#endif  // BFLBM_SPECTRUM_RING_H_
