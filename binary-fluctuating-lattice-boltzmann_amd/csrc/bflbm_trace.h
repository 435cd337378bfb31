// bflbm_trace.h -- ensemble traces: the droplet moments of every replica of a batch (or of a lone single-slab context)
// reduced into a device buffer every k steps on the owner's stream, read by the host once (include/bflbm.h, "Ensemble
// traces").  The per-lattice observables (bflbm_droplet_moments, bflbm_com_sums) cost a density pass, a reduction, a copy
// and a stream synchronisation per lattice and call; an ensemble sampled every step paid that B times per step.
// The sums are added in the order of bflbm_droplet.h (block_sum over 256 consecutive sites of the padded plane, the
// strided sum and tree of k_sum_partials per plane, the planes in sequence), so a record equals bflbm_droplet_moments
// of the same state bit for bit and does not depend on how the lattice is run.
// Included by bflbm.hip after bflbm_droplet.h (needs bflbm_ctx, bflbm_batch, block_sum).
#ifndef BFLBM_TRACE_H_
#define BFLBM_TRACE_H_

struct bflbm_trace {
  bflbm_ctx* ctx = nullptr;        // the owner: a lone context ...
  bflbm_batch* batch = nullptr;    // ... or a batch; both null once the owner is gone (detached)
  int device = 0;
  int nrep = 1;
  Geo G;
  int every = 1;
  long long capacity = 0;
  double threshold = 0.;
  long long since = 0;             // steps taken through the owner since creation or reset
  long long n = 0;                 // samples recorded
  double* d_rec = nullptr;         // [capacity][nrep][kNTrace]
  double* d_partial = nullptr;     // [nrep][nz][plane blocks][kNTrace]: stage 1 -> stage 2
  std::vector<long long> steps;    // [n][nrep]: every replica's step counter at the sample
};

namespace {

constexpr int kNTrace = BFLBM_TRACE_NREC;

// Stage 1 for one lattice: the f-density of the site as k_density forms it (19 pulled populations added in index
// order), its 12 terms, the workgroup's tree.  152 B read per site, nothing written per site; rho / phi of the owner are
// not touched.  `partial` is the lattice's own [nz][plane blocks][kNTrace].
__device__ __forceinline__ void trace_moments_body(const double* __restrict__ S, double* __restrict__ partial, const Geo& G, double threshold) {
  const long long s_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int p = (int)blockIdx.y;                       // single slab: storage plane == global z (H = 0)
  double v[kNTrace];
  for (int k = 0; k < kNTrace; ++k) v[k] = 0.;
  const int y = (int)(s_ / G.pitch);
  const int x = (int)(s_ - (long long)y * G.pitch);
  if (s_ < G.plane && x < G.nx) {
    SiteOff I; site_offsets(G, x, y, p, I);
    double fs[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) fs[i] = ld_sb(S + (long long)i * G.vol + I.pl[1 - Vel::cz[i]], I.o[1 - Vel::cy[i]][1 - Vel::cx[i]]);
    const double r = d_density(fs);
    v[10] = r;
    if (threshold == -INFINITY || r > threshold) {     // -inf: every cell, whatever its density is
      const int z = p;
      const double m[10] = { 1., (double)x, (double)y, (double)z, (double)x * x, (double)x * y, (double)x * z,
                             (double)y * y, (double)y * z, (double)z * z };
      for (int k = 0; k < 10; ++k) v[k] = r * m[k];
      v[11] = 1.;
    }
  }
  block_sum<kNTrace>(v, partial);
}

// grid (plane blocks, nz, 1): a lone context hands over its resident buffer
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

// Stages 2 and 3, one workgroup per replica: per plane the sum of k_sum_partials (every thread a 256-strided subsequence
// of the plane's block sums, then the tree), the planes added in sequence as reduce_blocks does on the host; the result
// goes straight into the sample's slot.  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_trace_finish(const double* __restrict__ partial, double* __restrict__ out, int nbx, int nplanes) {
  __shared__ double sh[kNTrace][256];
  const double* __restrict__ mine = partial + (long long)blockIdx.x * nplanes * nbx * kNTrace;
  double acc[kNTrace];
  for (int k = 0; k < kNTrace; ++k) acc[k] = 0.;
  for (int p = 0; p < nplanes; ++p) {
    double v[kNTrace];
    for (int k = 0; k < kNTrace; ++k) v[k] = 0.;
    const long long base = (long long)p * nbx;
    for (int b = threadIdx.x; b < nbx; b += 256) for (int k = 0; k < kNTrace; ++k) v[k] += mine[(base + b) * kNTrace + k];
    for (int k = 0; k < kNTrace; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) for (int k = 0; k < kNTrace; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
      __syncthreads();
    }
    // thread 0 reads only its own column here, and nobody reads a column again before the next plane's barrier
    if (threadIdx.x == 0) for (int k = 0; k < kNTrace; ++k) acc[k] += sh[k][0];
  }
  if (threadIdx.x == 0) for (int k = 0; k < kNTrace; ++k) out[(long long)blockIdx.x * kNTrace + k] = acc[k];
}

inline bool trace_attached(const bflbm_trace* t) { return t->ctx || t->batch; }
inline hipStream_t trace_stream(const bflbm_trace* t) { return t->ctx ? t->ctx->stream : t->batch->stream; }
inline bool trace_owner_open(const bflbm_trace* t) { return t->ctx && t->ctx->step_open(); }

// samples that `nsteps` more steps through the owner add
inline long long trace_due(const bflbm_trace* t, long long nsteps) { return (t->since + nsteps) / t->every - t->since / t->every; }
bool trace_overflows(const bflbm_trace* t, long long nsteps) { return t->n + trace_due(t, nsteps) > t->capacity; }

// enqueue the reduction of the resident state into slot n; no host synchronisation
int trace_record(bflbm_trace* t) {
  if (t->n >= t->capacity) return fail("trace full: %lld samples recorded (read it and bflbm_trace_reset, or create a larger one)", t->n);
  HIP_TRY(hipSetDevice(t->device));
  const Geo& G = t->G;
  const dim3 grid((unsigned)((G.plane + 255) / 256), (unsigned)G.nz, (unsigned)t->nrep);
  const hipStream_t stream = trace_stream(t);
  if (t->batch) {
    bflbm_batch* b = t->batch;
    if (batch_sync_table(b)) return 1;                 // a sample between steps (frame 0): the records may be stale
    hipLaunchKernelGGL(k_trace_moments_batch, grid, dim3(256), 0, stream, b->d_rec, t->d_partial, G, (int)b->k, t->threshold);
  } else {
    hipLaunchKernelGGL(k_trace_moments, grid, dim3(256), 0, stream, t->ctx->S[t->ctx->cur], t->d_partial, G, t->threshold);
  }
  HIP_TRY(hipGetLastError());
  double* slot = t->d_rec + (size_t)t->n * t->nrep * kNTrace;
  hipLaunchKernelGGL(k_trace_finish, dim3((unsigned)t->nrep), dim3(256), 0, stream, t->d_partial, slot, (int)grid.x, (int)grid.y);
  HIP_TRY(hipGetLastError());
  if (t->batch) for (const bflbm_ctx* c : t->batch->ctx) t->steps.push_back(c->steps);
  else t->steps.push_back(t->ctx->steps);
  t->n += 1;
  return 0;
}

int trace_after_step(bflbm_trace* t) {
  t->since += 1;
  return (t->since % t->every == 0) ? trace_record(t) : 0;
}

// the owner goes away: what was enqueued completes, the samples stay readable
void trace_detach(bflbm_trace* t) {
  hipSetDevice(t->device);
  (void)hipStreamSynchronize(trace_stream(t));
  if (t->ctx) t->ctx->trace = nullptr;
  if (t->batch) t->batch->trace = nullptr;
  t->ctx = nullptr; t->batch = nullptr;
}

int trace_create(bflbm_ctx* c, bflbm_batch* b, int every, long long capacity, double threshold, bflbm_trace** out) {
  const char* call = b ? "bflbm_batch_trace_create" : "bflbm_trace_create";
  if (every < 1) return fail("%s: every must be >= 1 (got %d)", call, every);
  if (capacity < 1) return fail("%s: capacity must be >= 1 (got %lld)", call, capacity);
  if (threshold != threshold) return fail("%s: the threshold is NaN (-INFINITY takes every cell)", call);
  if (c && c->batch) return fail("%s: the context is a replica of a batch; use bflbm_batch_trace_create on the batch", call);
  if (c && !c->G.zwrap) return fail("%s: a slab of a decomposed lattice (nranks > 1); traces take a lone single-slab context or a batch", call);
  if (c ? c->trace != nullptr : b->trace != nullptr) return fail("%s: the owner already has a trace", call);
  if (c && c->step_open()) return fail("%s inside an open step", call);
  const Geo& G = c ? c->G : b->G;
  const int nrep = c ? 1 : (int)b->ctx.size();
  const size_t rec_doubles_per_sample = (size_t)nrep * kNTrace;
  if ((unsigned long long)capacity > ((1ULL << 40) / sizeof(double)) / rec_doubles_per_sample)
    return fail("%s: capacity %lld x %d replicas exceeds 1 TB of records", call, capacity, nrep);
  const int device = c ? c->dom.device : b->device;
  HIP_TRY(hipSetDevice(device));
  const size_t nblocks = (size_t)((G.plane + 255) / 256) * (size_t)G.nz;
  bflbm_trace* t = new bflbm_trace();
  hipError_t e = hipMalloc((void**)&t->d_rec, (size_t)capacity * rec_doubles_per_sample * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_partial, nblocks * rec_doubles_per_sample * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (t->d_rec) hipFree(t->d_rec);
    delete t;
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  t->ctx = c; t->batch = b; t->device = device; t->nrep = nrep; t->G = G;
  t->every = every; t->capacity = capacity; t->threshold = threshold;
  if (c) c->trace = t; else b->trace = t;
  *out = t;
  return 0;
}

}  // namespace

extern "C" {

int bflbm_trace_create(bflbm_ctx* c, int every, long long capacity, double threshold, bflbm_trace** out) {
  if (!c || !out) return fail("bflbm_trace_create: null argument");
  return trace_create(c, nullptr, every, capacity, threshold, out);
}
int bflbm_batch_trace_create(bflbm_batch* b, int every, long long capacity, double threshold, bflbm_trace** out) {
  if (!b || !out) return fail("bflbm_batch_trace_create: null argument");
  return trace_create(nullptr, b, every, capacity, threshold, out);
}

int bflbm_trace_destroy(bflbm_trace* t) {
  if (!t) return 0;
  if (trace_attached(t)) trace_detach(t);              // waits for the reductions in flight: they write the buffers freed below
  hipSetDevice(t->device);
  if (t->d_rec) hipFree(t->d_rec);
  if (t->d_partial) hipFree(t->d_partial);
  delete t;
  return 0;
}

int bflbm_trace_sample(bflbm_trace* t) {
  if (!t) return fail("bflbm_trace_sample: null argument");
  if (!trace_attached(t)) return fail("bflbm_trace_sample: the owner of the trace was destroyed");
  if (trace_owner_open(t)) return fail("bflbm_trace_sample inside an open step");
  return trace_record(t);
}

int bflbm_trace_reset(bflbm_trace* t) {
  if (!t) return fail("bflbm_trace_reset: null argument");
  if (trace_attached(t) && trace_owner_open(t)) return fail("bflbm_trace_reset inside an open step");
  t->n = 0; t->since = 0;
  t->steps.clear();
  return 0;
}

int bflbm_trace_count(const bflbm_trace* t, long long* nsamples, int* nreplicas) {
  if (!t) return fail("bflbm_trace_count: null argument");
  if (nsamples) *nsamples = t->n;
  if (nreplicas) *nreplicas = t->nrep;
  return 0;
}

int bflbm_trace_read(bflbm_trace* t, long long first, long long count, double* rec, long long* steps) {
  if (!t) return fail("bflbm_trace_read: null argument");
  if (first < 0 || count < 0 || first > t->n || count > t->n - first)
    return fail("bflbm_trace_read: samples [%lld, %lld + %lld) of %lld recorded", first, first, count, t->n);
  if (count == 0) return 0;
  if (!rec) return fail("bflbm_trace_read: null argument");
  if (trace_attached(t) && trace_owner_open(t)) return fail("bflbm_trace_read inside an open step");
  HIP_TRY(hipSetDevice(t->device));
  const size_t per = (size_t)t->nrep * kNTrace;
  const double* src = t->d_rec + (size_t)first * per;
  const size_t nb = (size_t)count * per * sizeof(double);
  if (trace_attached(t)) {
    const hipStream_t stream = trace_stream(t);
    HIP_TRY(hipMemcpyAsync(rec, src, nb, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  } else {
    HIP_TRY(hipMemcpy(rec, src, nb, hipMemcpyDeviceToHost));   // detaching waited for everything enqueued
  }
  if (steps) std::copy(t->steps.begin() + (size_t)first * t->nrep, t->steps.begin() + (size_t)(first + count) * t->nrep, steps);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_TRACE_H_
