// bflbm_iface.h -- ensemble interface traces: the height of the `field = level` contour above every column (x, y) of every
// replica of a batch (or of a lone single-slab context), scanned along z on the device every k steps on the owner's
// stream and read by the host once (include/bflbm.h, "Interface traces": the definition is stated there and only there).
// It is the flat-interface observable of Flat_Interface.ipynb (cells 4, 7-9), which until now was a density pass, a
// full-field copy, a stream synchronisation and a numpy contour search per lattice and frame.
// The shape is that of bflbm_trace.h: stage 1 reads the resident populations (152 B per site, nothing written per site),
// stage 2 writes the sample's slot; rho / phi / density_valid of the owner are not touched.  No atomics, no LDS.
// The lifecycle and the sample store are those of bflbm_recorder.h; here are the kernels, their launch, the segment rule and
// the checks of the kind's own arguments.  Included by bflbm.hip after bflbm_trace.h (needs bflbm_ctx, bflbm_batch, batch_cus).
#ifndef BFLBM_IFACE_H_
#define BFLBM_IFACE_H_

struct bflbm_iface : bflbm_sample_store {  // d_rec [capacity][nrep][2][ny][nx], d_stage [nrep][nseg][2][padded plane]
  Geo G;
  int field = 0;                   // 0 rho (fluid f), 1 phi (fluid g)
  double level = 0.;
  int z_lo = 0, z_hi = 0;          // the window [z_lo, z_hi): pairs (z-1, z) for z = z_lo+1 ... z_hi-1
  int nseg = 1, seg_pairs = 1;     // stage 1 splits the pairs into nseg runs of seg_pairs (the last one ragged)
  bflbm_iface() : bflbm_sample_store("interface trace", "bflbm_iface") {}
  int record() override;
};

namespace {

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
  double prev = pull_density(F, G, I);
  double h[2] = { __builtin_nan(""), __builtin_nan("") };
  bool found[2] = { false, false };
  for (int z = za; z < zb; ++z) {
    I.pl[0] = I.pl[1]; I.pl[1] = I.pl[2];                               // the byte offsets inside a plane do not depend on z
    I.pl[2] = (long long)(z + 1 >= G.nzs ? 0 : z + 1) * G.plane;       // site_offsets' wrap with G.zwrap set: creation refuses other owners
    const double cur = pull_density(F, G, I);
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

// The segment count is the host's choice and changes no bit of a sample (a height depends only on its own pair, and
// stage 2 keeps the segment order).  Rule: the fewest segments that give stage 1 at least two workgroups per compute
// unit, each segment at least 4 pairs long, the last one ragged.  An unmeasured heuristic: nobody has timed other counts.
void iface_segments(const Geo& G, int nrep, int npairs, int ncu, int* nseg, int* seg_pairs) {
  const long long wgs = (long long)((G.plane + 255) / 256) * nrep;     // workgroups of one segment
  const long long want = (2LL * ncu + wgs - 1) / wgs;
  const long long most = std::max(1, npairs / 4);
  const int n0 = (int)std::min(want, most);
  *seg_pairs = (npairs + n0 - 1) / n0;
  *nseg = (npairs + *seg_pairs - 1) / *seg_pairs;
}

int iface_create(bflbm_ctx* c, bflbm_batch* b, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  const char* call = b ? "bflbm_batch_iface_create" : "bflbm_iface_create";
  const Geo& G = c ? c->G : b->G;
  if (field != 0 && field != 1) return fail("%s: field must be 0 (rho) or 1 (phi) (got %d)", call, field);
  if (level != level) return fail("%s: the level is NaN", call);
  if (z_lo < 0 || z_hi > G.nz || z_hi - z_lo < 2)
    return fail("%s: the window [%d, %d) must lie inside [0, %d) and hold at least two planes", call, z_lo, z_hi, G.nz);
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_iface_create", "interface trace")) return 1;
  const int nrep = c ? 1 : (int)b->ctx.size();
  std::unique_ptr<bflbm_iface> t(new bflbm_iface());
  t->G = G; t->field = field; t->level = level; t->z_lo = z_lo; t->z_hi = z_hi;
  iface_segments(G, nrep, z_hi - z_lo - 1, c ? c->ncu : batch_cus(b), &t->nseg, &t->seg_pairs);
  const std::string shape = " x 2 x " + std::to_string(G.ny) + " x " + std::to_string(G.nx) + " heights";
  if (store_attach(t.get(), c, b, call, every, capacity, (size_t)nrep * 2 * (size_t)G.ny * (size_t)G.nx,
                   (size_t)nrep * t->nseg * 2 * (size_t)G.plane, shape.c_str())) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// enqueue the scan of the resident state into slot n; no host synchronisation
int bflbm_iface::record() {
  if (store_begin(this)) return 1;
  const unsigned nbx = (unsigned)((G.plane + 255) / 256);
  const dim3 grid(nbx, (unsigned)nseg, (unsigned)nrep);
  const int npairs = z_hi - z_lo - 1;
  const hipStream_t stream = recorder_stream(this);
  if (batch) {
    if (batch_sync_table(batch)) return 1;             // a sample between steps (frame 0): the records may be stale
    hipLaunchKernelGGL(k_iface_scan_batch, grid, dim3(256), 0, stream, batch->d_rec, d_stage, G, (int)batch->k, field, level, z_lo, npairs, seg_pairs);
  } else {
    hipLaunchKernelGGL(k_iface_scan, grid, dim3(256), 0, stream, ctx->S[ctx->cur], d_stage, G, field, level, z_lo, npairs, seg_pairs);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_iface_finish, dim3(nbx, 2, (unsigned)nrep), dim3(256), 0, stream, d_stage, store_slot(this), G, nseg);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_iface_create(bflbm_ctx* c, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  if (!c || !out) return fail("bflbm_iface_create: null argument");
  return iface_create(c, nullptr, field, level, z_lo, z_hi, every, capacity, out);
}
int bflbm_batch_iface_create(bflbm_batch* b, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out) {
  if (!b || !out) return fail("bflbm_batch_iface_create: null argument");
  return iface_create(nullptr, b, field, level, z_lo, z_hi, every, capacity, out);
}

int bflbm_iface_destroy(bflbm_iface* t) { return store_destroy(t); }
int bflbm_iface_sample(bflbm_iface* t) { return store_sample(t, "bflbm_iface"); }
int bflbm_iface_reset(bflbm_iface* t) { return store_reset(t, "bflbm_iface"); }
int bflbm_iface_count(const bflbm_iface* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_iface", nsamples, nreplicas); }
int bflbm_iface_read(bflbm_iface* t, long long first, long long count, double* h, long long* steps) {
  return store_read(t, "bflbm_iface", first, count, h, steps);
}

int bflbm_iface_geometry(const bflbm_iface* t, int* nx, int* ny, int* nsegments, int* segment_pairs) {
  if (!t) return fail("bflbm_iface_geometry: null argument");
  if (nx) *nx = t->G.nx;
  if (ny) *ny = t->G.ny;
  if (nsegments) *nsegments = t->nseg;
  if (segment_pairs) *segment_pairs = t->seg_pairs;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_IFACE_H_
