// bflbm_iface.h -- ensemble interface traces: the height of the `field = level` contour above every column (x, y) of every
// replica of a batch (or of a lone single-slab context), scanned along z on the device every k steps on the owner's
// stream and read by the host once (include/bflbm.h, "Interface traces": the definition is stated there and only there).
// It is the flat-interface observable of Flat_Interface.ipynb (cells 4, 7-9), which until now was a density pass, a
// full-field copy, a stream synchronisation and a numpy contour search per lattice and frame.
// The shape is that of bflbm_trace.h: stage 1 reads the resident populations (152 B per site, nothing written per site),
// stage 2 writes the sample's slot; rho / phi / density_valid of the owner are not touched.  No atomics, no LDS.
// Included by bflbm.hip after bflbm_trace.h (needs bflbm_ctx, bflbm_batch, device_cus).
#ifndef BFLBM_IFACE_H_
#define BFLBM_IFACE_H_

struct bflbm_iface {
  bflbm_ctx* ctx = nullptr;        // the owner: a lone context ...
  bflbm_batch* batch = nullptr;    // ... or a batch; both null once the owner is gone (detached)
  int device = 0;
  int nrep = 1;
  Geo G;
  int field = 0;                   // 0 rho (fluid f), 1 phi (fluid g)
  double level = 0.;
  int z_lo = 0, z_hi = 0;          // the window [z_lo, z_hi): pairs (z-1, z) for z = z_lo+1 ... z_hi-1
  int nseg = 1, seg_pairs = 1;     // stage 1 splits the pairs into nseg runs of seg_pairs (the last one ragged)
  int every = 1;
  long long capacity = 0;
  long long since = 0;             // steps taken through the owner since creation or reset
  long long n = 0;                 // samples recorded
  double* d_h = nullptr;           // [capacity][nrep][2][ny][nx]
  double* d_partial = nullptr;     // [nrep][nseg][2][padded plane]: stage 1 -> stage 2
  std::vector<long long> steps;    // [n][nrep]: every replica's step counter at the sample
};

namespace {

// the 19 pulled populations of one fluid at the site I describes, added in index order: the double k_density stores
__device__ __forceinline__ double iface_density(const double* __restrict__ F, const Geo& G, const SiteOff& I) {
  double fs[Q];
#pragma unroll
  for (int i = 0; i < Q; ++i) fs[i] = ld_sb(F + (long long)i * G.vol + I.pl[1 - Vel::cz[i]], I.o[1 - Vel::cy[i]][1 - Vel::cx[i]]);
  return d_density(fs);
}

// Stage 1 for one lattice: the thread owns column (x, y) and marches up the pairs of its segment with d(z-1) kept in a
// register, so a segment of L pairs pulls L+1 planes; the rows of a plane are read coalesced along x.  It writes its first
// rising and first falling height, or a quiet NaN, to the lattice's own partial[segment][direction][padded plane].
// F = the first population of the chosen fluid (the g populations sit Q * vol behind the f populations).
__device__ __forceinline__ void iface_scan_body(const double* __restrict__ F, double* __restrict__ partial, const Geo& G,
                                                double level, int z_lo, int npairs, int seg_pairs) {
  const long long s_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int y = (int)(s_ / G.pitch);
  const int x = (int)(s_ - (long long)y * G.pitch);
  if (!(s_ < G.plane && x < G.nx)) return;
  const int seg = (int)blockIdx.y;
  const int za = z_lo + 1 + seg * seg_pairs;                            // the upper plane of the segment's first pair
  const int zb = min(za + seg_pairs, z_lo + 1 + npairs);                // one past the upper plane of its last pair
  SiteOff I; site_offsets(G, x, y, za - 1, I);                          // single slab: storage plane == global z (H = 0)
  double prev = iface_density(F, G, I);
  double h[2] = { __builtin_nan(""), __builtin_nan("") };
  bool found[2] = { false, false };
  for (int z = za; z < zb; ++z) {
    I.pl[0] = I.pl[1]; I.pl[1] = I.pl[2];                               // the byte offsets inside a plane do not depend on z
    I.pl[2] = (long long)(z + 1 >= G.nzs ? 0 : z + 1) * G.plane;       // site_offsets' wrap with G.zwrap set: creation refuses other owners
    const double cur = iface_density(F, G, I);
    const bool hit[2] = { prev < level && level <= cur, prev >= level && level > cur };   // false for a NaN density
#pragma unroll
    for (int d = 0; d < 2; ++d)
      if (hit[d] && !found[d]) { h[d] = (double)(z - 1) + (level - prev) / (cur - prev); found[d] = true; }
    prev = cur;
  }
  partial[(long long)(seg * 2 + 0) * G.plane + s_] = h[0];
  partial[(long long)(seg * 2 + 1) * G.plane + s_] = h[1];
}

// grid (plane blocks, segments, 1): a lone context hands over its resident buffer
__global__ void __launch_bounds__(256) k_iface_scan(const double* __restrict__ S, double* __restrict__ partial, Geo G, int field,
                                                    double level, int z_lo, int npairs, int seg_pairs) {
  iface_scan_body(S + (long long)field * Q * G.vol, partial, G, level, z_lo, npairs, seg_pairs);
}
// grid (plane blocks, segments, B): the replica's resident buffer from its record, as in k_trace_moments_batch
__global__ void __launch_bounds__(256) k_iface_scan_batch(const BatchRec* __restrict__ recs, double* __restrict__ partial, Geo G, int k,
                                                          int field, double level, int z_lo, int npairs, int seg_pairs) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  const long long per_replica = (long long)gridDim.y * 2 * G.plane;
  iface_scan_body(R->S[cur] + (long long)field * Q * G.vol, partial + (long long)blockIdx.z * per_replica, G, level, z_lo, npairs, seg_pairs);
}

// Stage 2, grid (plane blocks, 2, B): per replica, direction and column the first non-NaN candidate in segment order,
// written into the sample's dense [replica][2][ny][nx].  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_iface_finish(const double* __restrict__ partial, double* __restrict__ out, Geo G, int nseg) {
  const long long s_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int y = (int)(s_ / G.pitch);
  const int x = (int)(s_ - (long long)y * G.pitch);
  if (!(s_ < G.plane && x < G.nx)) return;
  const int dir = (int)blockIdx.y, rep = (int)blockIdx.z;
  const double* __restrict__ mine = partial + ((long long)rep * nseg * 2 + dir) * G.plane + s_;
  double h = __builtin_nan("");
  for (int seg = 0; seg < nseg; ++seg) {
    const double v = mine[(long long)seg * 2 * G.plane];
    if (v == v) { h = v; break; }
  }
  out[((long long)(rep * 2 + dir) * G.ny + y) * G.nx + x] = h;
}

inline bool iface_attached(const bflbm_iface* t) { return t->ctx || t->batch; }
inline hipStream_t iface_stream(const bflbm_iface* t) { return t->ctx ? t->ctx->stream : t->batch->stream; }
inline bool iface_owner_open(const bflbm_iface* t) { return t->ctx && t->ctx->step_open(); }
inline std::vector<bflbm_iface*>& iface_list(bflbm_iface* t) { return t->ctx ? t->ctx->ifaces : t->batch->ifaces; }
inline size_t iface_sample_doubles(const bflbm_iface* t) { return (size_t)t->nrep * 2 * (size_t)t->G.ny * (size_t)t->G.nx; }

// The segment count is the host's choice and changes no bit of a sample (a height depends only on its own pair, and
// stage 2 keeps the segment order).  Rule: the fewest segments that give stage 1 at least two workgroups per compute
// unit, each segment at least 4 pairs long, the last one ragged.  An unmeasured heuristic: nobody has timed other counts.
void iface_segments(const Geo& G, int nrep, int npairs, int* nseg, int* seg_pairs) {
  const long long wgs = (long long)((G.plane + 255) / 256) * nrep;     // workgroups of one segment
  const long long want = (2LL * device_cus() + wgs - 1) / wgs;
  const long long most = std::max(1, npairs / 4);
  const int n0 = (int)std::min(want, most);
  *seg_pairs = (npairs + n0 - 1) / n0;
  *nseg = (npairs + *seg_pairs - 1) / *seg_pairs;
}

// samples that `nsteps` more steps through the owner add
inline long long iface_due(const bflbm_iface* t, long long nsteps) { return (t->since + nsteps) / t->every - t->since / t->every; }
bool iface_overflows(const bflbm_iface* t, long long nsteps) { return t->n + iface_due(t, nsteps) > t->capacity; }

// enqueue the scan of the resident state into slot n; no host synchronisation
int iface_record(bflbm_iface* t) {
  if (t->n >= t->capacity) return fail("interface trace full: %lld samples recorded (read it and bflbm_iface_reset, or create a larger one)", t->n);
  HIP_TRY(hipSetDevice(t->device));
  const Geo& G = t->G;
  const unsigned nbx = (unsigned)((G.plane + 255) / 256);
  const dim3 grid(nbx, (unsigned)t->nseg, (unsigned)t->nrep);
  const int npairs = t->z_hi - t->z_lo - 1;
  const hipStream_t stream = iface_stream(t);
  if (t->batch) {
    bflbm_batch* b = t->batch;
    if (batch_sync_table(b)) return 1;                 // a sample between steps (frame 0): the records may be stale
    hipLaunchKernelGGL(k_iface_scan_batch, grid, dim3(256), 0, stream, b->d_rec, t->d_partial, G, (int)b->k, t->field, t->level, t->z_lo, npairs, t->seg_pairs);
  } else {
    hipLaunchKernelGGL(k_iface_scan, grid, dim3(256), 0, stream, t->ctx->S[t->ctx->cur], t->d_partial, G, t->field, t->level, t->z_lo, npairs, t->seg_pairs);
  }
  HIP_TRY(hipGetLastError());
  double* slot = t->d_h + (size_t)t->n * iface_sample_doubles(t);
  hipLaunchKernelGGL(k_iface_finish, dim3(nbx, 2, (unsigned)t->nrep), dim3(256), 0, stream, t->d_partial, slot, G, t->nseg);
  HIP_TRY(hipGetLastError());
  if (t->batch) for (const bflbm_ctx* c : t->batch->ctx) t->steps.push_back(c->steps);
  else t->steps.push_back(t->ctx->steps);
  t->n += 1;
  return 0;
}

int iface_after_step(bflbm_iface* t) {
  t->since += 1;
  return (t->since % t->every == 0) ? iface_record(t) : 0;
}

// the owner goes away: what was enqueued completes, the samples stay readable
void iface_detach(bflbm_iface* t) {
  hipSetDevice(t->device);
  (void)hipStreamSynchronize(iface_stream(t));
  std::vector<bflbm_iface*>& list = iface_list(t);
  list.erase(std::remove(list.begin(), list.end(), t), list.end());
  t->ctx = nullptr; t->batch = nullptr;
}

int iface_create(bflbm_ctx* c, bflbm_batch* b, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  const char* call = b ? "bflbm_batch_iface_create" : "bflbm_iface_create";
  const Geo& G = c ? c->G : b->G;
  if (field != 0 && field != 1) return fail("%s: field must be 0 (rho) or 1 (phi) (got %d)", call, field);
  if (level != level) return fail("%s: the level is NaN", call);
  if (z_lo < 0 || z_hi > G.nz || z_hi - z_lo < 2)
    return fail("%s: the window [%d, %d) must lie inside [0, %d) and hold at least two planes", call, z_lo, z_hi, G.nz);
  if (every < 1) return fail("%s: every must be >= 1 (got %d)", call, every);
  if (capacity < 1) return fail("%s: capacity must be >= 1 (got %lld)", call, capacity);
  if (c && c->batch) return fail("%s: the context is a replica of a batch; use bflbm_batch_iface_create on the batch", call);
  if (c && !c->G.zwrap) return fail("%s: a slab of a decomposed lattice (nranks > 1); interface traces take a lone single-slab context or a batch", call);
  if (c && c->step_open()) return fail("%s inside an open step", call);
  const int nrep = c ? 1 : (int)b->ctx.size();
  const size_t per_sample = (size_t)nrep * 2 * (size_t)G.ny * (size_t)G.nx;
  if ((unsigned long long)capacity > ((1ULL << 40) / sizeof(double)) / per_sample)
    return fail("%s: capacity %lld x %d replicas x 2 x %d x %d heights exceeds 1 TB of records", call, capacity, nrep, G.ny, G.nx);
  const int device = c ? c->dom.device : b->device;
  HIP_TRY(hipSetDevice(device));
  bflbm_iface* t = new bflbm_iface();
  t->nrep = nrep; t->G = G;
  iface_segments(G, nrep, z_hi - z_lo - 1, &t->nseg, &t->seg_pairs);
  hipError_t e = hipMalloc((void**)&t->d_h, (size_t)capacity * per_sample * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&t->d_partial, (size_t)nrep * t->nseg * 2 * (size_t)G.plane * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (t->d_h) hipFree(t->d_h);
    delete t;
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  t->ctx = c; t->batch = b; t->device = device;
  t->field = field; t->level = level; t->z_lo = z_lo; t->z_hi = z_hi;
  t->every = every; t->capacity = capacity;
  iface_list(t).push_back(t);
  *out = t;
  return 0;
}

}  // namespace

extern "C" {

int bflbm_iface_create(bflbm_ctx* c, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  if (!c || !out) return fail("bflbm_iface_create: null argument");
  return iface_create(c, nullptr, field, level, z_lo, z_hi, every, capacity, out);
}
int bflbm_batch_iface_create(bflbm_batch* b, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  if (!b || !out) return fail("bflbm_batch_iface_create: null argument");
  return iface_create(nullptr, b, field, level, z_lo, z_hi, every, capacity, out);
}

int bflbm_iface_destroy(bflbm_iface* t) {
  if (!t) return 0;
  if (iface_attached(t)) iface_detach(t);              // waits for the scans in flight: they write the buffers freed below
  hipSetDevice(t->device);
  if (t->d_h) hipFree(t->d_h);
  if (t->d_partial) hipFree(t->d_partial);
  delete t;
  return 0;
}

int bflbm_iface_sample(bflbm_iface* t) {
  if (!t) return fail("bflbm_iface_sample: null argument");
  if (!iface_attached(t)) return fail("bflbm_iface_sample: the owner of the interface trace was destroyed");
  if (iface_owner_open(t)) return fail("bflbm_iface_sample inside an open step");
  return iface_record(t);
}

int bflbm_iface_reset(bflbm_iface* t) {
  if (!t) return fail("bflbm_iface_reset: null argument");
  if (iface_attached(t) && iface_owner_open(t)) return fail("bflbm_iface_reset inside an open step");
  t->n = 0; t->since = 0;
  t->steps.clear();
  return 0;
}

int bflbm_iface_count(const bflbm_iface* t, long long* nsamples, int* nreplicas) {
  if (!t) return fail("bflbm_iface_count: null argument");
  if (nsamples) *nsamples = t->n;
  if (nreplicas) *nreplicas = t->nrep;
  return 0;
}

int bflbm_iface_geometry(const bflbm_iface* t, int* nx, int* ny, int* nsegments, int* segment_pairs) {
  if (!t) return fail("bflbm_iface_geometry: null argument");
  if (nx) *nx = t->G.nx;
  if (ny) *ny = t->G.ny;
  if (nsegments) *nsegments = t->nseg;
  if (segment_pairs) *segment_pairs = t->seg_pairs;
  return 0;
}

int bflbm_iface_read(bflbm_iface* t, long long first, long long count, double* h, long long* steps) {
  if (!t) return fail("bflbm_iface_read: null argument");
  if (first < 0 || count < 0 || first > t->n || count > t->n - first)
    return fail("bflbm_iface_read: samples [%lld, %lld + %lld) of %lld recorded", first, first, count, t->n);
  if (count == 0) return 0;
  if (!h) return fail("bflbm_iface_read: null argument");
  if (iface_attached(t) && iface_owner_open(t)) return fail("bflbm_iface_read inside an open step");
  HIP_TRY(hipSetDevice(t->device));
  const size_t per = iface_sample_doubles(t);
  const double* src = t->d_h + (size_t)first * per;
  const size_t nb = (size_t)count * per * sizeof(double);
  if (iface_attached(t)) {
    const hipStream_t stream = iface_stream(t);
    HIP_TRY(hipMemcpyAsync(h, src, nb, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  } else {
    HIP_TRY(hipMemcpy(h, src, nb, hipMemcpyDeviceToHost));     // detaching waited for everything enqueued
  }
  if (steps) std::copy(t->steps.begin() + (size_t)first * t->nrep, t->steps.begin() + (size_t)(first + count) * t->nrep, steps);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_IFACE_H_
