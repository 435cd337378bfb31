// bflbm_trace.h -- ensemble traces: the droplet moments of every replica of a batch (or of a lone single-slab context)
// reduced into a device buffer every k steps on the owner's stream, read by the host once (include/bflbm.h, "Ensemble
// traces").  The per-lattice observables (bflbm_droplet_moments, bflbm_com_sums) cost a density pass, a reduction, a copy
// and a stream synchronisation per lattice and call; an ensemble sampled every step paid that B times per step.
// The sums are added in the order of bflbm_reduce.h (block_reduce over 256 consecutive sites of the padded plane, the
// strided sum and tree of plane_reduce per plane, the planes in sequence), so a record equals bflbm_droplet_moments
// of the same state bit for bit and does not depend on how the lattice is run.
// The lifecycle and the sample store are those of bflbm_recorder.h; here are the kernels, their launch and the checks of
// the kind's own arguments.
// A ring of z-slabs: stage 1 runs on every slab's own stream over the slab's own planes (z the global plane index, the
// halo planes pulled through as the slab's density pass does) into [nzl][plane blocks][kNTrace] on the slab's device;
// slab 0 writes its planes straight into the stage buffer [nz][plane blocks][kNTrace] and takes every other slab's block
// to its planes' place there by the ring gather of bflbm_recorder.h; the same k_trace_finish then runs on slab 0.  The
// summation order is a lone context's, so with the bit-exact schedules the record equals the lone trace's bit for bit.
// Included by bflbm.hip after bflbm_droplet.h (needs bflbm_ctx, bflbm_batch, bflbm_ring, bflbm_reduce.h,
// batch_sync_table).  trace_moments_launch also serves the centre of mass of bflbm_shape.h and bflbm_radial.h.
#ifndef BFLBM_TRACE_H_
#define BFLBM_TRACE_H_

struct bflbm_trace : bflbm_sample_store {  // d_rec [capacity][nrep][kNTrace], d_stage [nrep][nz][plane blocks][kNTrace]
  Geo G;
  double threshold = 0.;
  RingGather gather;               // a ring: slab k's block is [nzl][plane blocks][kNTrace] (slab 0 writes d_stage itself)
  bflbm_trace() : bflbm_sample_store("trace", "bflbm_trace") {}
  int record() override;
  int record_ring();
};

namespace {

constexpr int kNTrace = BFLBM_TRACE_NREC;

// Stage 1 for one lattice: the f-density of the site as k_density forms it (19 pulled populations added in index
// order), its 12 terms, the workgroup's tree.  152 B read per site, nothing written per site; rho / phi of the owner are
// not touched.  `partial` is the lattice's own [nz][plane blocks][kNTrace].
__device__ __forceinline__ void trace_moments_body(const double* __restrict__ S, double* __restrict__ partial, const Geo& G, double threshold) {
  const PlaneSite st = plane_site(G, G.H);              // the own planes; a single slab: storage plane == global z (H = 0, z0 = 0)
  const int x = st.x, y = st.y, z = st.z;
  double v[kNTrace];
  for (int k = 0; k < kNTrace; ++k) v[k] = 0.;
  if (st.in) {
    SiteOff I; site_offsets(G, x, y, st.p, I);
    const double r = pull_density(S, G, I);
    v[10] = r;
    if (threshold == -INFINITY || r > threshold) {     // -inf: every cell, whatever its density is
      const double m[10] = { 1., (double)x, (double)y, (double)z, (double)x * x, (double)x * y, (double)x * z,
                             (double)y * y, (double)y * z, (double)z * z };
      for (int k = 0; k < 10; ++k) v[k] = r * m[k];
      v[11] = 1.;
    }
  }
  block_reduce<kNTrace>(v, partial);
}

// grid (plane blocks, own planes, 1): a lone context, or a slab of a ring, hands over its resident buffer
__global__ void __launch_bounds__(256) k_trace_moments(const double* __restrict__ S, double* __restrict__ partial, Geo G, double threshold) {
  trace_moments_body(S, partial, G, threshold);
}
// grid (plane blocks, nz, B): the replica's resident buffer from its record, as in k_density_batch
__global__ void __launch_bounds__(256) k_trace_moments_batch(const BatchRec* __restrict__ recs, double* __restrict__ partial, Geo G, int k, double threshold) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  const long long per_replica = (long long)gridDim.x * gridDim.y * kNTrace;
  trace_moments_body(R->S[cur], partial + (long long)blockIdx.z * per_replica, G, threshold);
}

// Stages 2 and 3, one workgroup per replica: per plane the sum of plane_reduce (every thread a 256-strided subsequence
// of the plane's block sums, then the tree), the planes added in sequence as slab_reduce does on the host; the result
// goes straight into the sample's slot.  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_trace_finish(const double* __restrict__ partial, double* __restrict__ out, int nbx, int nplanes) {
  const double* __restrict__ mine = partial + (long long)blockIdx.x * nplanes * nbx * kNTrace;
  double acc[kNTrace];
  for (int k = 0; k < kNTrace; ++k) acc[k] = 0.;
  for (int p = 0; p < nplanes; ++p) {
    const Column* sh = plane_reduce<kNTrace, SumRule>(mine + (long long)p * nbx * kNTrace, nbx);
    if (threadIdx.x == 0) for (int k = 0; k < kNTrace; ++k) acc[k] += sh[k][0];
  }
  if (threadIdx.x == 0) for (int k = 0; k < kNTrace; ++k) out[(long long)blockIdx.x * kNTrace + k] = acc[k];
}

int trace_create(bflbm_ctx* c, bflbm_batch* b, bflbm_ring* g, int every, long long capacity, double threshold, bflbm_trace** out) {
  const char* call = g ? "bflbm_ring_trace_create" : (b ? "bflbm_batch_trace_create" : "bflbm_trace_create");
  if (store_refuse_cadence(call, every, capacity)) return 1;
  if (threshold != threshold) return fail("%s: the threshold is NaN (-INFINITY takes every cell)", call);
  if (store_refuse_owner(c, call, "bflbm_batch_trace_create", "trace")) return 1;
  for (const bflbm_recorder* r : c ? c->recorders : (b ? b->recorders : g->recorders))
    if (dynamic_cast<const bflbm_trace*>(r)) return fail("%s: the owner already has a trace", call);
  std::unique_ptr<bflbm_trace> t(new bflbm_trace());
  t->G = c ? c->G : (b ? b->G : g->ctx[0]->G); t->threshold = threshold;
  const size_t per = (size_t)(b ? b->ctx.size() : 1) * kNTrace;
  const size_t nbx = (size_t)((t->G.plane + 255) / 256), nblocks = nbx * (size_t)t->G.nz;
  if (g) {
    if (ring_step_open(g)) return fail("%s inside an open step", call);
    const size_t plane_bytes = nbx * kNTrace * sizeof(double);
    HIP_TRY(gather_create(t->gather, g, [&](int k) { return (size_t)g->ctx[k]->nzl * plane_bytes; },
                          [&](int k) { return (size_t)g->ctx[k]->dom.z0 * plane_bytes; }));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, nblocks * per, "", g)) return 1;
  *out = t.release();
  return 0;
}

// The moments of a lone context (b null) or of the nrep replicas of a batch (c null) on `stream`: stage 1 into sums
// [nrep][nz][plane blocks][kNTrace], stages 2 and 3 into out [nrep][kNTrace].  What the trace records and what the shape
// and radial traces take their centre of mass from, so that it is Trace.com() of the same state bit for bit.
int trace_moments_launch(const bflbm_ctx* c, bflbm_batch* b, const Geo& G, int nrep, double threshold, double* sums, double* out,
                         hipStream_t stream) {
  const dim3 grid((unsigned)((G.plane + 255) / 256), (unsigned)G.nz, (unsigned)nrep);
  if (b) {
    if (batch_sync_table(b)) return 1;                 // a sample between steps (frame 0): the records may be stale; a fresh table enqueues nothing
    hipLaunchKernelGGL(k_trace_moments_batch, grid, dim3(256), 0, stream, b->d_rec, sums, G, (int)b->k, threshold);
  } else {
    hipLaunchKernelGGL(k_trace_moments, grid, dim3(256), 0, stream, c->S[c->cur], sums, G, threshold);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_trace_finish, dim3((unsigned)nrep), dim3(256), 0, stream, sums, out, (int)grid.x, (int)grid.y);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

// enqueue the reduction of the resident state into slot n; no host synchronisation
int bflbm_trace::record() {
  if (ring) return record_ring();
  if (store_begin(this)) return 1;
  if (trace_moments_launch(ctx, batch, G, nrep, threshold, d_stage, store_slot(this), recorder_stream(this))) return 1;
  store_recorded(this);
  return 0;
}

int bflbm_trace::record_ring() {
  if (store_begin(this)) return 1;
  const int n = (int)ring->ctx.size();
  const unsigned nbx = (unsigned)((G.plane + 255) / 256);
  for (int k = 0; k < n; ++k) {
    bflbm_ctx* c = ring->ctx[k];
    HIP_TRY(hipSetDevice(c->dom.device));
    if (gather_hold(gather, k, c->stream)) return 1;
    hipLaunchKernelGGL(k_trace_moments, dim3(nbx, (unsigned)c->nzl, 1), dim3(256), 0, c->stream,
                       c->S[c->cur], gather_target(gather, k, d_stage), c->G, threshold);
    HIP_TRY(hipGetLastError());
    if (gather_ready(gather, k, c->stream)) return 1;
  }
  HIP_TRY(hipSetDevice(device));
  const hipStream_t s0 = ring->ctx[0]->stream;
  if (gather_take(gather, d_stage, s0)) return 1;
  hipLaunchKernelGGL(k_trace_finish, dim3(1), dim3(256), 0, s0, d_stage, store_slot(this), (int)nbx, G.nz);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_trace_create(bflbm_ctx* c, int every, long long capacity, double threshold, bflbm_trace** out) {
  if (!c || !out) return fail("bflbm_trace_create: null argument");
  return trace_create(c, nullptr, nullptr, every, capacity, threshold, out);
}
int bflbm_batch_trace_create(bflbm_batch* b, int every, long long capacity, double threshold, bflbm_trace** out) {
  if (!b || !out) return fail("bflbm_batch_trace_create: null argument");
  return trace_create(nullptr, b, nullptr, every, capacity, threshold, out);
}
int bflbm_ring_trace_create(bflbm_ring* r, int every, long long capacity, double threshold, bflbm_trace** out) {
  if (!r || !out) return fail("bflbm_ring_trace_create: null argument");
  if (r->ctx.size() == 1) return bflbm_trace_create(r->ctx[0], every, capacity, threshold, out);   // the whole box: the lone trace of ctx[0]
  return trace_create(nullptr, nullptr, r, every, capacity, threshold, out);
}

int bflbm_trace_destroy(bflbm_trace* t) { return store_destroy(t); }
int bflbm_trace_sample(bflbm_trace* t) { return store_sample(t, "bflbm_trace"); }
int bflbm_trace_reset(bflbm_trace* t) { return store_reset(t, "bflbm_trace"); }
int bflbm_trace_count(const bflbm_trace* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_trace", nsamples, nreplicas); }
int bflbm_trace_read(bflbm_trace* t, long long first, long long count, double* rec, long long* steps) {
  return store_read(t, "bflbm_trace", first, count, rec, steps);
}

}  // extern "C"

#endif  // BFLBM_TRACE_H_
