// bflbm_spectrum_ring.h -- the spectrum trace of a ring of z-slabs (include/bflbm.h, "Spectrum traces"): bins, weights
// and normalisation are those of bflbm_spectrum.h, the transform is the slab FFT of bflbm_sf_ring.h.  Slab d owns the
// rows ky in [ny d / n, ny (d+1) / n) of the half spectrum.  A sample is, without a host synchronisation,
//   1. on every slab's stream      observe_launch into the scratch buffer, one batched 2-D D2Z per distinct variable
//                                  into h2[var][nzl][ny][nxc], the event `planes`;
//   2. on every slab's stream      after the other slabs' `planes`: k_spectrum_collect gathers the slab's rows of every
//                                  plane of every slab into zb[var][nz][nky][nxc], reading the sources' h2 in place, where
//                                  every source is on the same device or peer-mapped and neither the ring's transport nor
//                                  BFLBM_RING_COPY_FALLBACK=1 asks for copies; the strided copies of
//                                  bflbm_ring_sf_accumulate otherwise (the same doubles); the event `collected`;
//   3. on every slab's stream      batched Z2Z along z in place, k_spectrum_bin and k_spectrum_finish as they are with
//                                  the slab's own tables (spectrum_tables::build_slab) into the slab's sums [pair][bin];
//   4. on slab 0's stream          the ring gather of bflbm_recorder.h: the slabs' sums into d_stage[slab][pair][bin], then
//                                  k_spectrum_combine adds the slabs in the order 0 ... n-1 into the slot.
// What the next sample overwrites while another stream may still read it waits the other way round: a slab's 2-D
// transforms for every other slab's `collected`, a slab's sums for the gather's `taken`.  A record depends on the spectra,
// the slabs' tables and the slab count alone.  No atomics, no LDS beyond the tree of k_spectrum_bin, no scratch.
// Included by bflbm.hip after bflbm_spectrum.h (needs bflbm_ring, ring_prepare_ref, ring_force_copies, load_fft_many,
// fields_observe_slab).
#ifndef BFLBM_SPECTRUM_RING_H_
#define BFLBM_SPECTRUM_RING_H_

namespace {

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
  const int nx = G.nx, ny = G.ny, nz = G.nz, nxc = nx / 2 + 1;
  if (ny < n) return fail("%s: fewer rows (ny = %d) than slabs (%d)", call, ny, n);
  if (load_fft_many()) return 1;

  std::unique_ptr<bflbm_spectrum> t(new bflbm_spectrum());
  spectrum_select(t.get(), G, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg);
  {                                                        // bins, count and q are the whole box's: a lone trace's
    spectrum_tables::Tables T;
    spectrum_tables::build(nx, ny, nz, kind, t->zero_avg, L, spectrum_tables::kChunkLen, T);
    t->nbins = T.nbins; t->count = T.count; t->q = T.q;
  }
  const size_t nv = t->vars.size();
  const size_t per = (size_t)npairs * (size_t)t->nbins, sb = per * sizeof(double);   // a slab's bin sums: its block of the gather
  t->slab.resize((size_t)n);
  t->nchunks = 0; t->max_chunks_per_bin = 0;
  std::vector<SpectrumSrc> src((size_t)n);
  for (int d = 0; d < n; ++d) {
    bflbm_ctx* c = g->ctx[d];
    SpectrumSlab& q = t->slab[d];
    q.device = c->dom.device;
    q.ky0 = (int)((long long)ny * d / n); q.ky1 = (int)((long long)ny * (d + 1) / n);
    const int nky = q.ky1 - q.ky0;
    q.nk = (long long)nz * nky * nxc;
    spectrum_tables::Tables T;
    spectrum_tables::build_slab(nx, ny, nz, q.ky0, q.ky1, kind, t->zero_avg, L, spectrum_tables::kChunkLen, T);
    q.nchunks = (long long)T.chunks.size();
    t->nchunks += q.nchunks; t->max_chunks_per_bin = std::max(t->max_chunks_per_bin, T.max_chunks_per_bin);
    HIP_TRY(hipSetDevice(q.device));
    const size_t hb = nv * (size_t)c->nzl * ny * nxc * sizeof(double2), zb = nv * (size_t)q.nk * sizeof(double2);
    const size_t lb_ = std::max<size_t>(T.list.size(), 1) * sizeof(uint32_t);
    const size_t cb = std::max<size_t>(T.chunks.size(), 1) * sizeof(spectrum_tables::Chunk), bb = T.bin_first.size() * sizeof(int);
    const size_t pb = (size_t)npairs * std::max<size_t>(T.chunks.size(), 1) * sizeof(double);
    hipError_t e = hipMalloc((void**)&q.h2, hb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.zb, zb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.d_list, lb_);
    if (e == hipSuccess) e = hipMalloc((void**)&q.d_chunks, cb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.d_bin_first, bb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.partial, pb);
    if (e == hipSuccess) e = hipMalloc((void**)&q.d_src, (size_t)n * sizeof(SpectrumSrc));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail("%s: out of device memory on slab %d (plane spectra %zu + row spectra %zu + index list %zu + chunk table %zu + bin table %zu + chunk sums %zu + bin sums %zu bytes): %s",
                  call, d, hb, zb, lb_, cb, bb, pb, sb, hipGetErrorString(e));
    }
    if (!T.list.empty()) HIP_TRY(hipMemcpy(q.d_list, T.list.data(), T.list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!T.chunks.empty()) HIP_TRY(hipMemcpy(q.d_chunks, T.chunks.data(), T.chunks.size() * sizeof(spectrum_tables::Chunk), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(q.d_bin_first, T.bin_first.data(), bb, hipMemcpyHostToDevice));
    for (hipEvent_t* ev : {&q.planes, &q.collected}) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    int n2[2] = { ny, nx };
    if (g_fftm.plan_many(&q.plan2d, 2, n2, nullptr, 1, ny * nx, nullptr, 1, ny * nxc, HIPFFT_D2Z, c->nzl) != HIPFFT_SUCCESS) {
      q.plan2d = nullptr;
      return fail("%s: the hipFFT plan failed for the %d planes of %d x %d of slab %d", call, c->nzl, nx, ny, d);
    }
    int n1[1] = { nz }, emb[1] = { nz };
    const int col = nky * nxc;                             // columns of one variable: the stride between the elements of a column
    if (g_fftm.plan_many(&q.plan1d, 1, n1, emb, col, 1, emb, col, 1, HIPFFT_Z2Z, col) != HIPFFT_SUCCESS) {
      q.plan1d = nullptr;
      return fail("%s: the hipFFT plan failed for the %d columns of %d of slab %d", call, col, nz, d);
    }
    src[(size_t)d] = SpectrumSrc{ q.h2, c->dom.z0, c->nzl };
  }
  // the source table on every slab, and whether its kernels may read every source in place (the rule of ring_copy)
  for (int d = 0; d < n; ++d) {
    SpectrumSlab& q = t->slab[d];
    HIP_TRY(hipSetDevice(q.device));
    HIP_TRY(hipMemcpy(q.d_src, src.data(), (size_t)n * sizeof(SpectrumSrc), hipMemcpyHostToDevice));
    q.reachable = true;
    for (int s = 0; s < n; ++s) {
      const int pd = t->slab[s].device;
      if (pd == q.device) continue;
      int can = 0; hipDeviceCanAccessPeer(&can, q.device, pd);
      bool ok = false;
      if (can) { const hipError_t pe = hipDeviceEnablePeerAccess(pd, 0); ok = (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled); }
      (void)hipGetLastError();
      q.reachable = q.reachable && ok;
    }
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
  const int n = (int)g->ctx.size(), nxc = nx / 2 + 1;
  const size_t nv = vars.size();
  if (fs.source != 1 && ring_prepare_ref(g)) return 1;                // the global centre of mass: the slabs' own prepare_ref is then a no-op
  const bool in_place = !ring_force_copies() && g->transport == 0;
  // 1. observe + 2-D transforms of the own planes
  for (int k = 0; k < n; ++k) {
    bflbm_ctx* c = g->ctx[k];
    SpectrumSlab& q = slab[k];
    HIP_TRY(hipSetDevice(q.device));
    for (int d = 0; d < n; ++d) if (d != k) HIP_TRY(hipStreamWaitEvent(c->stream, slab[d].collected, 0));   // the last sample's h2 was taken
    const double* dense;                                  // [comp][z local][y][x]
    if (fields_observe_slab(c, fs, "spectrum trace sample", &dense)) return 1;
    const long long nloc = (long long)c->nzl * c->G.dplane;
    g_fft.set_stream(q.plan2d, c->stream);
    for (size_t v = 0; v < nv; ++v)
      if (g_fft.exec_d2z(q.plan2d, const_cast<double*>(dense) + (long long)vars[v] * nloc,
                         (hipfftDoubleComplex*)(q.h2 + (long long)v * c->nzl * ny * nxc)) != HIPFFT_SUCCESS)
        return fail("spectrum trace: hipfftExecD2Z (planes of slab %d) failed", k);
    HIP_TRY(hipEventRecord(q.planes, c->stream));
  }
  // 2. the transpose and 3. the z transforms and the binning of the own rows
  const double inv_n = 1.0 / (double)nsites;
  for (int d = 0; d < n; ++d) {
    bflbm_ctx* c = g->ctx[d];
    SpectrumSlab& q = slab[d];
    const int nky = q.ky1 - q.ky0;
    const long long run = (long long)nky * nxc;
    HIP_TRY(hipSetDevice(q.device));
    for (int s = 0; s < n; ++s) if (s != d) HIP_TRY(hipStreamWaitEvent(c->stream, slab[s].planes, 0));
    if (in_place && q.reachable) {
      hipLaunchKernelGGL(k_spectrum_collect, dim3((unsigned)((run + 255) / 256), (unsigned)nz, (unsigned)nv), dim3(256), 0, c->stream,
                         q.d_src, n, q.zb, ny, nz, q.ky0, nky, nxc);
      HIP_TRY(hipGetLastError());
    } else {
      for (int s = 0; s < n; ++s) {
        const bflbm_ctx* cs = g->ctx[s];
        for (size_t v = 0; v < nv; ++v) {
          const double2* from = slab[s].h2 + ((long long)v * cs->nzl * ny + q.ky0) * nxc;              // plane 0 of slab s, row ky0
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
      if (g_fftm.exec_z2z(q.plan1d, p, p, HIPFFT_FORWARD) != HIPFFT_SUCCESS) return fail("spectrum trace: hipfftExecZ2Z (columns of slab %d) failed", d);
    }
    if (q.nchunks > 0) {
      hipLaunchKernelGGL(k_spectrum_bin, dim3((unsigned)q.nchunks, (unsigned)pairs.n, 1), dim3(256), 0, c->stream,
                         q.zb, q.d_list, q.d_chunks, q.partial, q.nk, nspec, nx, pairs, inv_n);
      HIP_TRY(hipGetLastError());
    }
    if (gather_hold(gather, d, c->stream)) return 1;
    hipLaunchKernelGGL(k_spectrum_finish, dim3((unsigned)((nbins + 255) / 256), (unsigned)pairs.n, 1), dim3(256), 0, c->stream,
                       q.partial, q.d_bin_first, gather_target(gather, d, d_stage), nbins, std::max(q.nchunks, 1LL));
    HIP_TRY(hipGetLastError());
    if (gather_ready(gather, d, c->stream)) return 1;
  }
  // 4. slab 0 takes the sums and adds them in slab order
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
