// bflbm_hist.h -- histogram traces: the counts of the sites of chosen hydrovs, hydrovsbar or noise components over fixed
// bins, and of chosen pairs of them over the product of two binnings, recorded on the device as a time series of 64-bit
// integers for a lone single-slab context, every replica of a batch or a ring of z-slabs (include/bflbm.h, "Histogram
// traces": the binning rule and the layout of a sample are stated there and only there).  The velocity PDF against
// Maxwell-Boltzmann, P(rho) and P(phi) turning bimodal while a mixture demixes, the occupancy of the (rho, phi) plane and
// "is the field still finite, and how wide is it" (the reference's Debug.H:136-228) are distributions; without this a
// user downloads whole fields per replica and sample and bins them on the host.
// A sample is, on the owner's stream(s) and without a host synchronisation,
//   the accumulators' observation   exactly as the profile trace takes it (fields_observe / fields_observe_slab),
//   k_hist_count<NV, CCAP>          the counting launch, grid (groups, 1, replicas), 256 threads: every workgroup keeps all
//                                   C counters of its replica as 32-bit words in LDS (CCAP = 4096 or 16384 of them: 16 or
//                                   64 KiB), strides over the tiles of 2048 consecutive sites of the replica's dense
//                                   volume, loads a site's variables once (a thread takes two neighbouring sites, one
//                                   16-byte access where the volume is 16-byte aligned), derives every bin index and
//                                   every pair cell from those registers and adds 1 to each counter in LDS; at the
//                                   end one 64-bit global integer add per non-zero counter into totals [replica][C],
//   k_hist_finish                   the finishing launch: the totals into the slot [sample][replica][C], and the totals
//                                   back to zero for the next sample.
// Integer sums commute, so the record is exact whatever the launch geometry.  The groups are chosen on the host so that
// no workgroup meets 2^31 sites: its 32-bit counters cannot wrap before the flush.  How the partial counts reach the
// finishing launch: the global-add form ships; a [groups][C] stage buffer was not built (it writes and reads
// groups x C words whatever the field, the adds touch the non-zero counters only).  Adds to one LDS address serialise
// and a zero-noise mixture puts a whole wave into one bin; one add per run of equal counters within a wave was built and
// measured against the plain add and lost, so the plain add ships.
// A ring: every slab counts its own planes on its own stream into its own totals and finishes them into its own [C] block;
// slab 0 takes the blocks side by side into `incoming` (the ring gather of bflbm_recorder.h) and adds them into the slot.
// Not built on purpose: automatic ranges or adaptive bins, running minima and maxima, weighted histograms, fusing the
// counting into the observation kernels, a noise source on batches, histograms over more than two variables.
// Host part: plain C++17 beside field_select that needs bflbm_fieldsel.h's host part and a declared int fail(const char*,
// ...): the argument refusals, the block layout and the scales.  A stand-alone program defines BFLBM_HIST_HOST_ONLY (and
// BFLBM_FIELDSEL_HOST_ONLY) and includes it after bflbm_fieldsel.h (tests/hist_main.cpp).  HIP part: the lifecycle and
// the sample store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by bflbm.hip after
// bflbm_profile.h (needs bflbm_ctx, bflbm_batch, bflbm_ring, FieldSelection, fields_observe, field_dispatch_nv,
// ring_prepare_ref, fstat_aligned).
#ifndef BFLBM_HIST_H_
#define BFLBM_HIST_H_

#include <cmath>

namespace hist_limits {
constexpr int kMaxVars = fstat_limits::kMaxVars;
constexpr int kMaxPairs = 4;
constexpr int kMaxBins = 4096;
constexpr int kMaxCounters = 16384;  // 64 KiB of 32-bit counters: two workgroups in a CU's 160 KiB of LDS
constexpr int kSmallCounters = 4096; // the smaller of the two LDS sizes the counting kernel is compiled for
constexpr int kTile = 2048;          // sites per work item: 256 threads x 4 turns x 2 neighbouring sites
constexpr int kGroups = 512;         // workgroups of a counting launch over all replicas (two per CU of 256)
constexpr long long kMaxTilesPerGroup = 1LL << 20;   // x kTile = 2^31 sites: a 32-bit counter cannot wrap
}

// the binnings and the blocks of a sample; a by-value kernel parameter
struct HistLayout {
  int nvars, npairs, C;
  int nbins[hist_limits::kMaxVars];
  int voff[hist_limits::kMaxVars];   // variable v: nbins[v] bins, then below, above, nan
  double lo[hist_limits::kMaxVars], scale[hist_limits::kMaxVars];
  int pa[hist_limits::kMaxPairs], pb[hist_limits::kMaxPairs];
  int poff[hist_limits::kMaxPairs];  // pair p: nbins[pa] x nbins[pb] cells in row-major order, then outside ...
  int pout[hist_limits::kMaxPairs];  // ... at this counter
  // what the kernel forms a pair's cell from without picking a slot: cell = sum over v of bin_v * pmul[p][v] (nbins[pb]
  // for v = pa, 1 for v = pb, else 0); bit p of vpairs[v]: pair p uses slot v, and is `outside` where bin_v is no bin
  int pmul[hist_limits::kMaxPairs][hist_limits::kMaxVars];
  int vpairs[hist_limits::kMaxVars];
};

namespace {

// What every creation call refuses about its source, variables, ranges, bins and pairs, in the order of include/bflbm.h.
int hist_refuse_args(const char* call, int source, int nvars, const int* vars, const double* lo, const double* hi, const int* nbins,
                     int npairs, const int* pair_a, const int* pair_b) {
  using namespace hist_limits;
  if (npairs < 0 || npairs > kMaxPairs) return fail("%s: 0..%d pairs (got %d)", call, kMaxPairs, npairs);
  if (field_refuse_args(call, source, 2, nvars, vars, npairs, pair_a, pair_b)) return 1;
  if (!lo || !hi || !nbins) return fail("%s: null argument", call);
  long long total = 0;
  for (int v = 0; v < nvars; ++v) {
    if (!std::isfinite(lo[v]) || !std::isfinite(hi[v]) || !(hi[v] > lo[v]))
      return fail("%s: variable slot %d: the range needs finite lo < hi (got %.17g, %.17g)", call, v, lo[v], hi[v]);
    if (nbins[v] < 1 || nbins[v] > kMaxBins) return fail("%s: variable slot %d: 1..%d bins (got %d)", call, v, kMaxBins, nbins[v]);
    const double scale = (double)nbins[v] / (hi[v] - lo[v]);
    if (!std::isfinite(scale) || !(scale > 0.))
      return fail("%s: variable slot %d: the scale nbins / (hi - lo) = %g is not finite and positive", call, v, scale);
    total += nbins[v] + 3;
  }
  for (int p = 0; p < npairs; ++p) {
    if (pair_a[p] == pair_b[p]) return fail("%s: pair %d: slot %d with itself", call, p, pair_a[p]);
    total += (long long)nbins[pair_a[p]] * nbins[pair_b[p]] + 1;
  }
  if (total > kMaxCounters) return fail("%s: %lld counters per replica exceed %d", call, total, kMaxCounters);
  return 0;
}

// the layout of accepted arguments
HistLayout hist_layout(int nvars, const double* lo, const double* hi, const int* nbins, int npairs, const int* pair_a, const int* pair_b) {
  using namespace hist_limits;
  HistLayout L;
  L.nvars = nvars; L.npairs = npairs;
  int at = 0;
  for (int v = 0; v < kMaxVars; ++v) {
    const bool in = v < nvars;
    L.nbins[v] = in ? nbins[v] : 1;
    L.lo[v] = in ? lo[v] : 0.;
    L.scale[v] = in ? (double)nbins[v] / (hi[v] - lo[v]) : 1.;
    L.voff[v] = at;
    if (in) at += nbins[v] + 3;
  }
  for (int p = 0; p < kMaxPairs; ++p) {
    const bool in = p < npairs;
    L.pa[p] = in ? pair_a[p] : 0; L.pb[p] = in ? pair_b[p] : 0;
    L.poff[p] = at;
    if (in) at += L.nbins[L.pa[p]] * L.nbins[L.pb[p]] + 1;
    L.pout[p] = in ? at - 1 : 0;
  }
  for (int v = 0; v < kMaxVars; ++v) {
    L.vpairs[v] = 0;
    for (int p = 0; p < kMaxPairs; ++p) {
      const bool a = p < npairs && L.pa[p] == v, b = p < npairs && L.pb[p] == v;
      L.pmul[p][v] = a ? L.nbins[L.pb[p]] : (b ? 1 : 0);
      if (a || b) L.vpairs[v] |= 1 << p;
    }
  }
  L.C = at;
  return L;
}

// offset and length of block k: the variables in order, then the pairs
inline int hist_block_offset(const HistLayout& L, int k) { return k < L.nvars ? L.voff[k] : L.poff[k - L.nvars]; }
inline int hist_block_length(const HistLayout& L, int k) {
  if (k < L.nvars) return L.nbins[k] + 3;
  const int p = k - L.nvars;
  return L.nbins[L.pa[p]] * L.nbins[L.pb[p]] + 1;
}

// the LDS counters of the instantiation that serves C, and the workgroups per replica of a counting launch over `sites`
// dense sites of each of `nrep` replicas
inline int hist_lds_counters(int C) { return C <= hist_limits::kSmallCounters ? hist_limits::kSmallCounters : hist_limits::kMaxCounters; }
inline long long hist_tiles(long long sites) { return (sites + hist_limits::kTile - 1) / hist_limits::kTile; }
inline long long hist_groups(long long sites, int nrep) {
  using namespace hist_limits;
  const long long tiles = hist_tiles(sites);
  const long long want = std::min<long long>(tiles, std::max(1, kGroups / nrep));
  return std::max(want, (tiles + kMaxTilesPerGroup - 1) / kMaxTilesPerGroup);
}

}  // namespace

#ifndef BFLBM_HIST_HOST_ONLY

#include <memory>
#include <string>
#include <vector>

struct bflbm_hist : bflbm_sample_store {     // d_rec [capacity][nrep][C] as long long, d_stage: the totals [nrep][C]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar, 2 noise
  HistLayout L;
  double* fields = nullptr;         // a batch: [nrep][nvars][nsites]
  // a ring: slab k > 0 counts into slab_totals[k] [C] on its device and finishes them into its block [C] of the gather,
  // which slab 0 receives in incoming [nslabs - 1][C]
  RingGather gather;
  std::vector<unsigned long long*> slab_totals;
  long long* incoming = nullptr;
  bflbm_hist() : bflbm_sample_store("histogram trace", "bflbm_hist") {}
  ~bflbm_hist() override {
    for (size_t k = 1; k < slab_totals.size(); ++k)
      if (slab_totals[k]) { hipSetDevice(gather.part[k].device); hipFree(slab_totals[k]); }
    if (fields || incoming) hipSetDevice(device);
    if (fields) hipFree(fields);
    if (incoming) hipFree(incoming);
  }
  unsigned long long* totals() const { return reinterpret_cast<unsigned long long*>(d_stage); }
  int record() override;
  int record_ring();
  int count(const double* dense, long long rep_stride, long long comp_stride, long long sites, int reps,
            unsigned long long* into, hipStream_t stream) const;
};

namespace {

// the counter of variable v for the site value x: the binning rule of include/bflbm.h, the subtraction first, the
// multiplication second (the build never contracts them)
__device__ __forceinline__ int hist_bin(double x, double lo, double scale, int nbins) {
  const double d = x - lo;
  const double t = d * scale;
  if (t != t) return nbins + 2;
  if (t < 0.) return nbins;
  if (t >= (double)nbins) return nbins + 1;
  return (int)t;
}

// One LDS add per site and counter; idx < 0: no site.  Measured against one add per run of equal counters within a wave
// (the lane that starts a run adds its length): no faster on scattered bins, nor where every lane meets the same counter
// (DESIGN.md section 8), so the plain form ships.
__device__ __forceinline__ void hist_add(unsigned* __restrict__ sh, int idx) {
  if (idx >= 0) atomicAdd(&sh[idx], 1u);
}

// grid (groups, 1, replicas), 256 threads.  fields: the dense volumes, variable v of replica r at
// fields + r rep_stride + V.vol[v] comp_stride, `sites` doubles; totals: [replica][C].  NV, the number of variables, and
// CCAP, the LDS counters, are template parameters.
template <int NV, int CCAP>
__global__ void __launch_bounds__(256) k_hist_count(const double* __restrict__ fields, long long rep_stride, long long comp_stride,
                                                    long long sites, unsigned long long* __restrict__ totals, FstatVars V, HistLayout L) {
  using namespace hist_limits;
  __shared__ unsigned sh[CCAP];
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < L.C; i += 256) sh[i] = 0u;
  __syncthreads();
  const double* vol[NV];
  bool al[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    vol[v] = fields + (long long)blockIdx.z * rep_stride + (long long)V.vol[v] * comp_stride;
    al[v] = fstat_aligned(vol[v]);
  }
  const long long tiles = (sites + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll 2
    for (int turn = 0; turn < kTile / 512; ++turn) {
      const long long s = tile * kTile + turn * 512 + 2 * tid;      // even: the pair (s, s + 1)
      const bool in0 = s < sites, in1 = s + 1 < sites;
      int cell0[kMaxPairs], cell1[kMaxPairs];             // a pair's cell, formed while the variables pass by
      int out0 = 0, out1 = 0;                               // bit p: a coordinate of pair p is no bin
#pragma unroll
      for (int p = 0; p < kMaxPairs; ++p) { cell0[p] = 0; cell1[p] = 0; }
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        double x0 = 0., x1 = 0.;
        if (in1 && al[v]) { const double2 m = *reinterpret_cast<const double2*>(vol[v] + s); x0 = m.x; x1 = m.y; }
        else { if (in0) x0 = vol[v][s]; if (in1) x1 = vol[v][s + 1]; }
        const int nb = L.nbins[v];
        const int i0 = hist_bin(x0, L.lo[v], L.scale[v], nb), i1 = hist_bin(x1, L.lo[v], L.scale[v], nb);
        hist_add(sh, in0 ? L.voff[v] + i0 : -1);
        hist_add(sh, in1 ? L.voff[v] + i1 : -1);
        out0 |= i0 >= nb ? L.vpairs[v] : 0;
        out1 |= i1 >= nb ? L.vpairs[v] : 0;
#pragma unroll
        for (int p = 0; p < kMaxPairs; ++p) {
          if (p < L.npairs) { cell0[p] += i0 * L.pmul[p][v]; cell1[p] += i1 * L.pmul[p][v]; }
        }
      }
#pragma unroll
      for (int p = 0; p < kMaxPairs; ++p) {
        if (p < L.npairs) {
          hist_add(sh, in0 ? ((out0 >> p) & 1 ? L.pout[p] : L.poff[p] + cell0[p]) : -1);
          hist_add(sh, in1 ? ((out1 >> p) & 1 ? L.pout[p] : L.poff[p] + cell1[p]) : -1);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long* __restrict__ mine = totals + (long long)blockIdx.z * L.C;
  for (int i = tid; i < L.C; i += 256) {
    const unsigned n = sh[i];
    if (n) atomicAdd(&mine[i], (unsigned long long)n);
  }
}

// grid (ceil(n / 256)), n = replicas x C: the totals into `out` and back to zero.  `more`: nmore further blocks of n
// counts each, added in order (slab 0 of a ring: the other slabs' blocks).
__global__ void __launch_bounds__(256) k_hist_finish(unsigned long long* __restrict__ totals, long long* __restrict__ out, int n,
                                                     const long long* __restrict__ more, int nmore) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  long long s = (long long)totals[i];
  totals[i] = 0ull;
  for (int k = 0; k < nmore; ++k) s += more[(long long)k * n + i];
  out[i] = s;
}

int hist_create(bflbm_ctx* c, bflbm_batch* b, bflbm_ring* g, int source, int nvars, const int* vars, const double* lo, const double* hi,
                const int* nbins, int npairs, const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_hist** out) {
  const char* call = b ? "bflbm_batch_hist_create" : (g ? "bflbm_ring_hist_create" : "bflbm_hist_create");
  if (hist_refuse_args(call, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b)) return 1;
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_hist_create", "histogram trace")) return 1;
  if (b && source == 2) return fail("%s: the observation of a batch has no noise form; source 2 needs a lone context or a ring", call);
  if (recorder_refuse_open(c, b, g, call)) return 1;
  const Geo& G = c ? c->G : (b ? b->G : g->ctx[0]->G);

  std::unique_ptr<bflbm_hist> t(new bflbm_hist());
  recorder_bind(t.get(), c, b, every, g);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  t->L = hist_layout(nvars, lo, hi, nbins, npairs, pair_a, pair_b);

  const size_t per = (size_t)t->nrep * t->L.C;
  const std::string shape = " x " + std::to_string(t->L.C) + " counters";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the fields of a batch
  const size_t sb = per * sizeof(long long);
  const size_t fb = b ? (size_t)t->nrep * nvars * (size_t)t->nsites * sizeof(double) : 0;
  const size_t cb = (size_t)t->L.C * sizeof(long long);      // a ring: one slab's block
  const size_t ib = g ? (g->ctx.size() - 1) * cb : 0;
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e == hipSuccess && g) {
    e = hipMalloc((void**)&t->incoming, ib);
    if (e == hipSuccess) e = gather_create(t->gather, g, [&](int) { return cb; }, [&](int k) { return (size_t)(k - 1) * cb; });
    if (e == hipSuccess) t->slab_totals.resize(g->ctx.size(), nullptr);
    for (size_t k = 1; k < t->slab_totals.size() && e == hipSuccess; ++k) {   // zeroed on the slab's stream, ahead of its first count
      e = hipSetDevice(t->gather.part[k].device);
      if (e == hipSuccess) e = hipMalloc((void**)&t->slab_totals[k], cb);
      if (e == hipSuccess) e = hipMemsetAsync(t->slab_totals[k], 0, cb, g->ctx[k]->stream);
    }
  }
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (fields %zu bytes, slab blocks %zu each, incoming %zu; then records %zu x %lld + totals %zu): %s",
                call, fb, g ? 2 * cb : (size_t)0, ib, sb, capacity, sb, hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, per, shape.c_str(), g)) return 1;
  // The totals are the store's stage buffer, so their zeroing comes after the owner's list took the trace: its failure
  // detaches again (store_destroy), as the upload of the shape trace's directions does.
  bflbm_hist* h = t.release();
  e = hipMemsetAsync(h->d_stage, 0, sb, recorder_stream(h));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(h);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = h;
  return 0;
}

}  // namespace

// the counting launch over `sites` dense sites of each of `reps` replicas on `stream`
int bflbm_hist::count(const double* dense, long long rep_stride, long long comp_stride, long long sites, int reps,
                      unsigned long long* into, hipStream_t stream) const {
  using namespace hist_limits;
  const dim3 grid((unsigned)hist_groups(sites, reps), 1, (unsigned)reps);
  const bool small = hist_lds_counters(L.C) == kSmallCounters;
  if (!field_dispatch_nv(fs.nvars, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if (small) hipLaunchKernelGGL((k_hist_count<NV, kSmallCounters>), grid, dim3(256), 0, stream, dense, rep_stride, comp_stride, sites, into, fs.vol, L);
        else hipLaunchKernelGGL((k_hist_count<NV, kMaxCounters>), grid, dim3(256), 0, stream, dense, rep_stride, comp_stride, sites, into, fs.vol, L);
      })) return fail("histogram trace: %d variables", fs.nvars);
  HIP_TRY(hipGetLastError());
  return 0;
}

// enqueue the observation, the counting and the finishing launch of the resident state into slot n; no host synchronisation
int bflbm_hist::record() {
  if (ring) return record_ring();
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "histogram trace sample", &dense, &rep_stride)) return 1;
  if (count(dense, rep_stride, nsites, nsites, nrep, totals(), stream)) return 1;
  const int n = nrep * L.C;
  hipLaunchKernelGGL(k_hist_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     totals(), reinterpret_cast<long long*>(store_slot(this)), n, (const long long*)nullptr, 0);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

int bflbm_hist::record_ring() {
  if (store_begin(this)) return 1;
  if (fs.source != 1 && ring_prepare_ref(ring)) return 1;  // the global centre of mass: the slabs' own prepare_ref is then a no-op
  const int n = (int)ring->ctx.size();
  const long long plane = (long long)nx * ny;
  const unsigned fin = (unsigned)((L.C + 255) / 256);
  for (int k = 0; k < n; ++k) {
    bflbm_ctx* c = ring->ctx[k];
    const double* dense;
    if (fields_observe_slab(c, fs, "histogram trace sample", &dense)) return 1;        // selects the slab's device
    const long long sites = (long long)c->nzl * plane;
    if (count(dense, 0, sites, sites, 1, k > 0 ? slab_totals[k] : totals(), c->stream)) return 1;
    if (k > 0) {
      if (gather_hold(gather, k, c->stream)) return 1;
      hipLaunchKernelGGL(k_hist_finish, dim3(fin), dim3(256), 0, c->stream, slab_totals[k], static_cast<long long*>(gather.part[k].block), L.C,
                         (const long long*)nullptr, 0);
      HIP_TRY(hipGetLastError());
      if (gather_ready(gather, k, c->stream)) return 1;
    }
  }
  HIP_TRY(hipSetDevice(device));
  const hipStream_t s0 = ring->ctx[0]->stream;
  if (gather_take(gather, incoming, s0)) return 1;
  hipLaunchKernelGGL(k_hist_finish, dim3(fin), dim3(256), 0, s0, totals(), reinterpret_cast<long long*>(store_slot(this)), L.C,
                     (const long long*)incoming, n - 1);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_hist_create(bflbm_ctx* c, int source, int nvars, const int* vars, const double* lo, const double* hi, const int* nbins,
                      int npairs, const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_hist** out) {
  if (!c || !vars || !out) return fail("bflbm_hist_create: null argument");
  return hist_create(c, nullptr, nullptr, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b, every, capacity, out);
}
int bflbm_batch_hist_create(bflbm_batch* b, int source, int nvars, const int* vars, const double* lo, const double* hi, const int* nbins,
                            int npairs, const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_hist** out) {
  if (!b || !vars || !out) return fail("bflbm_batch_hist_create: null argument");
  return hist_create(nullptr, b, nullptr, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b, every, capacity, out);
}
int bflbm_ring_hist_create(bflbm_ring* r, int source, int nvars, const int* vars, const double* lo, const double* hi, const int* nbins,
                           int npairs, const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_hist** out) {
  if (!r || !vars || !out) return fail("bflbm_ring_hist_create: null argument");
  if (r->ctx.size() == 1)                                  // the whole box: the lone recorder of ctx[0], served by its steps
    return hist_create(r->ctx[0], nullptr, nullptr, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b, every, capacity, out);
  return hist_create(nullptr, nullptr, r, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b, every, capacity, out);
}

int bflbm_hist_destroy(bflbm_hist* t) { return store_destroy(t); }
int bflbm_hist_sample(bflbm_hist* t) { return store_sample(t, "bflbm_hist"); }
int bflbm_hist_reset(bflbm_hist* t) { return store_reset(t, "bflbm_hist"); }
int bflbm_hist_count(const bflbm_hist* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_hist", nsamples, nreplicas); }
int bflbm_hist_read(bflbm_hist* t, long long first, long long count, long long* counts, long long* steps) {
  return store_read(t, "bflbm_hist", first, count, reinterpret_cast<double*>(counts), steps);   // 8-byte slots, copied bit for bit
}

int bflbm_hist_geometry(const bflbm_hist* t, int* ncounters, int* nblocks, int* offsets, int* lengths, int* tile_sites, int* groups,
                        int* lds_counters) {
  if (!t) return fail("bflbm_hist_geometry: null argument");
  const int nb = t->L.nvars + t->L.npairs;
  if (ncounters) *ncounters = t->L.C;
  if (nblocks) *nblocks = nb;
  for (int k = 0; k < nb; ++k) {
    if (offsets) offsets[k] = hist_block_offset(t->L, k);
    if (lengths) lengths[k] = hist_block_length(t->L, k);
  }
  if (tile_sites) *tile_sites = hist_limits::kTile;
  if (groups) *groups = (int)hist_groups(t->nsites, t->nrep);
  if (lds_counters) *lds_counters = hist_lds_counters(t->L.C);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_HIST_HOST_ONLY

#endif  // BFLBM_HIST_H_
