// bflbm_shape.h -- shape traces: the radius at which the `field = level` surface of a droplet is met along fixed rays from
// a centre, for every replica of a batch (or a lone single-slab context), found on the device every k steps on the
// owner's stream and read by the host once (include/bflbm.h, "Shape traces": the definition is stated there and only there).
// It is the droplet-shape observable of Droplet_Fluctuation.ipynb (cells 32, 38, 41), which extracts a marching-cubes
// surface per frame on the host and expands its radius in spherical harmonics; the projection of the radii onto Y_lm is
// a small host product (analysis.shape_modes).  It is the interface trace turned from columns into rays.
// Stages, all on the owner's stream, no atomics, no LDS of their own, nothing of the owner written:
//   1. with a null centre: trace_moments_launch of bflbm_trace.h into the recorder's own [nrep][12],
//      so the centre is Trace.com() of the same state bit for bit;
//   2. k_shape_density(_batch): the chosen field's density of every site into the recorder's own padded [nrep][nzs][plane]
//      (152 B read, 8 B written per site), so that a sample point costs 8 doubles and not 8 x 19 populations;
//   3. k_shape_rays: one ray per lane, the pairs (k-1, k) split into segments, every work item writes its first candidate;
//   4. k_shape_finish: per ray the first non-NaN candidate in segment order, and the centre, into the sample's slot.
// The lifecycle and the sample store are those of bflbm_recorder.h.  Included by bflbm.hip after bflbm_iface.h (needs
// bflbm_ctx, bflbm_batch, batch_cus, trace_moments_launch).
#ifndef BFLBM_SHAPE_H_
#define BFLBM_SHAPE_H_

// d_rec [capacity][nrep][3 + ndir]; d_stage = dirs [ndir][3] | density [nrep][nzs * plane] | candidates [nrep][nseg][ndir]
//                                             | moments [nrep][12] | block sums [nrep][nz][plane blocks][12]  (the last two: null centre)
struct bflbm_shape : bflbm_sample_store {
  Geo G;
  int field = 0;                   // 0 rho (fluid f), 1 phi (fluid g)
  double level = 0.;
  int direction = 0;               // 0 falling outward, 1 rising outward
  bool com = false;                // the centre is the centre of mass of the cells above `threshold`
  double centre[3] = { 0., 0., 0. };
  double threshold = 0.;
  int ndir = 0, nsteps = 0;
  double step = 0.;
  int nseg = 1, seg_len = 1;       // stage 3 splits the pairs k = 1 ... nsteps into nseg runs of seg_len (the last one ragged)
  bflbm_shape() : bflbm_sample_store("shape trace", "bflbm_shape") {}
  size_t density_doubles() const { return (size_t)G.nzs * (size_t)G.plane; }
  double* d_dirs() const { return d_stage; }
  double* d_density() const { return d_dirs() + 3 * (size_t)ndir; }
  double* d_cand() const { return d_density() + (size_t)nrep * density_doubles(); }
  double* d_moments() const { return d_cand() + (size_t)nrep * nseg * ndir; }
  double* d_sums() const { return d_moments() + (size_t)nrep * kNTrace; }
  int record() override;
};

namespace {

constexpr int kShapeLanes = 64;    // one wave per workgroup of the ray kernel: the most workgroups a ray count gives

// Stage 2 for one lattice: the density of the site as k_density forms it, into the recorder's padded copy.
__device__ __forceinline__ void shape_density_body(const double* __restrict__ F, double* __restrict__ dens, const Geo& G) {
  const long long s_ = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int y = (int)(s_ / G.pitch);
  const int x = (int)(s_ - (long long)y * G.pitch);
  if (!(s_ < G.plane && x < G.nx)) return;
  const int p = (int)blockIdx.y;                                         // single slab: storage plane == global z (H = 0)
  SiteOff I; site_offsets(G, x, y, p, I);
  dens[(long long)p * G.plane + s_] = pull_density(F, G, I);
}

// grid (plane blocks, nz, 1): a lone context hands over its resident buffer
__global__ void __launch_bounds__(256) k_shape_density(const double* __restrict__ S, double* __restrict__ dens, Geo G, int field) {
  shape_density_body(S + (long long)field * Q * G.vol, dens, G);
}
// grid (plane blocks, nz, B): the replica's resident buffer from its record, as in k_trace_moments_batch
__global__ void __launch_bounds__(256) k_shape_density_batch(const BatchRec* __restrict__ recs, double* __restrict__ dens, Geo G, int k, int field) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  shape_density_body(R->S[cur] + (long long)field * Q * G.vol, dens + (long long)blockIdx.z * G.nzs * G.plane, G);
}

// the centre of a replica: c_a = m_a / m_0 of its moments (0 / 0 = NaN where no cell is above the threshold), or the fixed one
__device__ __forceinline__ void shape_centre(const double* __restrict__ moments, int rep, double fx, double fy, double fz, double (&c)[3]) {
  c[0] = fx; c[1] = fy; c[2] = fz;
  if (moments) {
    const double* __restrict__ m = moments + (long long)rep * kNTrace;
    const double m0 = m[0];
    c[0] = m[1] / m0; c[1] = m[2] / m0; c[2] = m[3] / m0;
  }
}

// the lower corner index of one axis wrapped into [0, n), and its upper neighbour's
__device__ __forceinline__ void shape_wrap(int i, int n, int& lo, int& hi) {
  lo = i % n;
  if (lo < 0) lo += n;
  hi = lo + 1 == n ? 0 : lo + 1;
}

// The density at c + t u, trilinearly interpolated in the stated order.  A point with a coordinate that is not below 2^30
// in magnitude (a NaN or infinite centre among them) has the density NaN, and no index is formed from it: the loads then
// go to site 0 and their values are dropped.
__device__ __forceinline__ double shape_density_at(const double* __restrict__ dens, const Geo& G, const double (&c)[3],
                                                   const double (&u)[3], double t) {
  const double px = c[0] + t * u[0], py = c[1] + t * u[1], pz = c[2] + t * u[2];
  const bool ok = fabs(px) < 0x1p30 && fabs(py) < 0x1p30 && fabs(pz) < 0x1p30;   // false for a NaN
  const double qx = ok ? px : 0., qy = ok ? py : 0., qz = ok ? pz : 0.;
  const double flx = floor(qx), fly = floor(qy), flz = floor(qz);
  const double fx = qx - flx, fy = qy - fly, fz = qz - flz;
  int x0, x1, y0, y1, z0, z1;
  shape_wrap((int)flx, G.nx, x0, x1);
  shape_wrap((int)fly, G.ny, y0, y1);
  shape_wrap((int)flz, G.nzs, z0, z1);                                   // single slab: nzs == nz
  const double* __restrict__ r00 = dens + (long long)z0 * G.plane + (long long)y0 * G.pitch;
  const double* __restrict__ r10 = dens + (long long)z0 * G.plane + (long long)y1 * G.pitch;
  const double* __restrict__ r01 = dens + (long long)z1 * G.plane + (long long)y0 * G.pitch;
  const double* __restrict__ r11 = dens + (long long)z1 * G.plane + (long long)y1 * G.pitch;
  const double d000 = r00[x0], d100 = r00[x1], d010 = r10[x0], d110 = r10[x1];
  const double d001 = r01[x0], d101 = r01[x1], d011 = r11[x0], d111 = r11[x1];
  const double c00 = d000 + fx * (d100 - d000), c10 = d010 + fx * (d110 - d010);
  const double c01 = d001 + fx * (d101 - d001), c11 = d011 + fx * (d111 - d011);
  const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
  const double d = c0 + fz * (c1 - c0);
  return ok ? d : __builtin_nan("");
}

// Stage 3, grid (ray blocks, segments, B): the lane owns ray j and marches outward over the pairs of its segment with
// d_{k-1} kept in a register, so a segment of L pairs interpolates L+1 points.  No lane leaves the loop early: a wave
// issues every load of its segment whatever its lanes have found.  It writes its first candidate, or a quiet NaN, to
// cand[replica][segment][ray].
__global__ void __launch_bounds__(kShapeLanes) k_shape_rays(const double* __restrict__ dens, const double* __restrict__ dirs,
                                                            const double* __restrict__ moments, double* __restrict__ cand, Geo G,
                                                            double cx, double cy, double cz, double level, int rising,
                                                            int ndir, double step, int nsteps, int seg_len) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= ndir) return;
  const int seg = (int)blockIdx.y, rep = (int)blockIdx.z;
  double c[3];
  shape_centre(moments, rep, cx, cy, cz, c);
  const double u[3] = { dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2] };
  const double* __restrict__ mine = dens + (long long)rep * G.nzs * G.plane;
  const int ka = 1 + seg * seg_len;                                      // the outer point of the segment's first pair
  const int kb = min(ka + seg_len, nsteps + 1);                          // one past the outer point of its last pair
  double prev = shape_density_at(mine, G, c, u, (double)(ka - 1) * step);
  double r = __builtin_nan("");
  bool found = false;
  for (int k = ka; k < kb; ++k) {
    const double cur = shape_density_at(mine, G, c, u, (double)k * step);
    const bool hit = rising ? (prev < level && level <= cur) : (prev >= level && level > cur);   // false for a NaN density
    const double num = rising ? level - prev : prev - level;
    const double den = rising ? cur - prev : prev - cur;
    if (hit && !found) { r = step * ((double)(k - 1) + num / den); found = true; }
    prev = cur;
  }
  cand[((long long)rep * gridDim.y + seg) * ndir + j] = r;
}

// Stage 4, grid (blocks over 3 + ndir, B): entry e < 3 of a replica's sample is the centre used, entry 3 + j the first
// non-NaN candidate of ray j in segment order.  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_shape_finish(const double* __restrict__ cand, const double* __restrict__ moments,
                                                      double* __restrict__ out, double cx, double cy, double cz, int ndir, int nseg) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= 3 + ndir) return;
  const int rep = (int)blockIdx.y;
  double v = __builtin_nan("");
  if (e < 3) {
    double c[3];
    shape_centre(moments, rep, cx, cy, cz, c);
    v = e == 0 ? c[0] : (e == 1 ? c[1] : c[2]);
  } else {
    const double* __restrict__ mine = cand + (long long)rep * nseg * ndir + (e - 3);
    for (int seg = 0; seg < nseg; ++seg) {
      const double w = mine[(long long)seg * ndir];
      if (w == w) { v = w; break; }
    }
  }
  out[(long long)rep * (3 + ndir) + e] = v;
}

// The segment count is the host's choice and changes no bit of a sample (a radius depends only on its own pair, and
// stage 4 keeps the segment order).  Rule: the fewest segments that give stage 3 at least one wave per SIMD (4 per
// compute unit), each segment at least 4 pairs long, the last one ragged.  An unmeasured heuristic, like the one-wave
// workgroups of stage 3: nobody has timed other counts or launch shapes.
void shape_segments(int nrep, int ndir, int nsteps, int ncu, int* nseg, int* seg_len) {
  const long long wgs = (long long)((ndir + kShapeLanes - 1) / kShapeLanes) * nrep;   // workgroups of one segment
  const long long want = (4LL * ncu + wgs - 1) / wgs;
  const long long most = std::max(1, nsteps / 4);
  const int n0 = (int)std::min(want, most);
  *seg_len = (nsteps + n0 - 1) / n0;
  *nseg = (nsteps + *seg_len - 1) / *seg_len;
}

int shape_create(bflbm_ctx* c, bflbm_batch* b, int field, double level, int direction, const double* centre, double threshold,
                 int ndir, const double* dirs, double step, int nsteps, int every, long long capacity, bflbm_shape** out) {
  const char* call = b ? "bflbm_batch_shape_create" : "bflbm_shape_create";
  if (!dirs) return fail("%s: null argument", call);
  if (field != 0 && field != 1) return fail("%s: field must be 0 (rho) or 1 (phi) (got %d)", call, field);
  if (direction != 0 && direction != 1) return fail("%s: direction must be 0 (falling outward) or 1 (rising outward) (got %d)", call, direction);
  if (level != level) return fail("%s: the level is NaN", call);
  if (!centre && threshold != threshold) return fail("%s: the threshold is NaN (-INFINITY takes every cell)", call);
  if (centre && !(std::isfinite(centre[0]) && std::isfinite(centre[1]) && std::isfinite(centre[2])))
    return fail("%s: the fixed centre is not finite", call);
  if (ndir < 1 || ndir > 65536) return fail("%s: ndir must be in 1 ... 65536 (got %d)", call, ndir);
  for (int j = 0; j < ndir; ++j) {
    const double* u = dirs + 3 * (size_t)j;
    const double uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    if (!(std::fabs(uu - 1.) <= 1e-6))                                   // a non-finite component fails here too
      return fail("%s: direction %d is not a unit vector (|u.u - 1| <= 1e-6, finite components)", call, j);
  }
  if (!(std::isfinite(step) && step > 0.)) return fail("%s: step must be finite and > 0 (got %g)", call, step);
  if (nsteps < 1) return fail("%s: nsteps must be >= 1 (got %d)", call, nsteps);
  if (store_refuse_cadence(call, every, capacity) || store_refuse_owner(c, call, "bflbm_batch_shape_create", "shape trace")) return 1;
  const Geo& G = c ? c->G : b->G;
  const int nrep = c ? 1 : (int)b->ctx.size();
  std::unique_ptr<bflbm_shape> t(new bflbm_shape());
  t->G = G; t->field = field; t->level = level; t->direction = direction; t->threshold = threshold;
  t->com = !centre;
  if (centre) std::copy(centre, centre + 3, t->centre);
  t->ndir = ndir; t->step = step; t->nsteps = nsteps;
  shape_segments(nrep, ndir, nsteps, c ? c->ncu : batch_cus(b), &t->nseg, &t->seg_len);
  const size_t nbx = (size_t)((G.plane + 255) / 256);
  const size_t stage = 3 * (size_t)ndir + (size_t)nrep * (t->density_doubles() + (size_t)t->nseg * ndir)
                     + (t->com ? (size_t)nrep * kNTrace * (1 + nbx * (size_t)G.nz) : 0);
  const std::string shape = " x (3 + " + std::to_string(ndir) + ") radii";
  if (store_attach(t.get(), c, b, call, every, capacity, (size_t)nrep * (3 + (size_t)ndir), stage, shape.c_str())) return 1;
  bflbm_shape* s = t.release();
  const hipError_t e = hipMemcpy(s->d_dirs(), dirs, 3 * (size_t)ndir * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(s);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = s;
  return 0;
}

}  // namespace

// enqueue the four stages on the resident state into slot n; no host synchronisation
int bflbm_shape::record() {
  if (store_begin(this)) return 1;
  const unsigned nbx = (unsigned)((G.plane + 255) / 256);
  const dim3 sites(nbx, (unsigned)G.nz, (unsigned)nrep);
  const hipStream_t stream = recorder_stream(this);
  if (batch && batch_sync_table(batch)) return 1;                        // for k_shape_density_batch: between steps (frame 0) the records may be stale
  if (com && trace_moments_launch(ctx, batch, G, nrep, threshold, d_sums(), d_moments(), stream)) return 1;
  if (batch) hipLaunchKernelGGL(k_shape_density_batch, sites, dim3(256), 0, stream, batch->d_rec, d_density(), G, (int)batch->k, field);
  else hipLaunchKernelGGL(k_shape_density, sites, dim3(256), 0, stream, ctx->S[ctx->cur], d_density(), G, field);
  HIP_TRY(hipGetLastError());
  const double* moments = com ? d_moments() : nullptr;
  hipLaunchKernelGGL(k_shape_rays, dim3((unsigned)((ndir + kShapeLanes - 1) / kShapeLanes), (unsigned)nseg, (unsigned)nrep), dim3(kShapeLanes), 0, stream,
                     d_density(), d_dirs(), moments, d_cand(), G, centre[0], centre[1], centre[2], level, direction, ndir, step, nsteps, seg_len);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_shape_finish, dim3((unsigned)((3 + ndir + 255) / 256), (unsigned)nrep), dim3(256), 0, stream,
                     d_cand(), moments, store_slot(this), centre[0], centre[1], centre[2], ndir, nseg);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_shape_create(bflbm_ctx* c, int field, double level, int direction, const double* centre_or_null, double threshold,
                       int ndir, const double* dirs, double step, int nsteps, int every, long long capacity, bflbm_shape** out) {
  if (!c || !out) return fail("bflbm_shape_create: null argument");
  return shape_create(c, nullptr, field, level, direction, centre_or_null, threshold, ndir, dirs, step, nsteps, every, capacity, out);
}
int bflbm_batch_shape_create(bflbm_batch* b, int field, double level, int direction, const double* centre_or_null, double threshold,
                             int ndir, const double* dirs, double step, int nsteps, int every, long long capacity, bflbm_shape** out) {
  if (!b || !out) return fail("bflbm_batch_shape_create: null argument");
  return shape_create(nullptr, b, field, level, direction, centre_or_null, threshold, ndir, dirs, step, nsteps, every, capacity, out);
}

int bflbm_shape_destroy(bflbm_shape* t) { return store_destroy(t); }
int bflbm_shape_sample(bflbm_shape* t) { return store_sample(t, "bflbm_shape"); }
int bflbm_shape_reset(bflbm_shape* t) { return store_reset(t, "bflbm_shape"); }
int bflbm_shape_count(const bflbm_shape* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_shape", nsamples, nreplicas); }
int bflbm_shape_read(bflbm_shape* t, long long first, long long count, double* r, long long* steps) {
  return store_read(t, "bflbm_shape", first, count, r, steps);
}

int bflbm_shape_geometry(const bflbm_shape* t, int* ndir, int* nsteps, int* nsegments, int* segment_len) {
  if (!t) return fail("bflbm_shape_geometry: null argument");
  if (ndir) *ndir = t->ndir;
  if (nsteps) *nsteps = t->nsteps;
  if (nsegments) *nsegments = t->nseg;
  if (segment_len) *segment_len = t->seg_len;
  return 0;
}

}  // extern "C"

#endif  // BFLBM_SHAPE_H_
