// bflbm_reduce.h -- the one reduction layer of the slab observables: how a slab's resident density becomes a handful
// of doubles (mass, centre of mass, droplet moments, both droplet fits, the total-density bound of `auto`, the moments
// of the trace, shape and radial recorders).  Every sum has one fixed order, restated in numpy by tests/exact_sums.py:
//   stage 1  one partial per 256 consecutive sites of the padded plane: block_reduce (the workgroup tree);
//   stage 2  per plane, every thread a 256-strided subsequence of the plane's block partials, then the tree: plane_reduce;
//   fold     on the host, either every block partial in block order (Fold::HostBlocks) or the per-plane results of
//            stage 2 plane by plane (Fold::Planes): slab_reduce.
// The device part needs Geo only; slab_reduce needs bflbm_ctx, plane_grid, ensure_density, fail and HIP_TRY.
// Included by bflbm.hip.
#ifndef BFLBM_REDUCE_H_
#define BFLBM_REDUCE_H_

namespace {

// ---- the combining rules: combine(k, a, b) of value k, and what an empty sequence of value k gives ------------------
struct SumRule {
  static __host__ __device__ double combine(int, double a, double b) { return a + b; }
  static __host__ __device__ double empty(int) { return 0.; }
};
struct MinMaxRule {              // value 0 the minimum, value 1 the maximum
  static __host__ __device__ double combine(int k, double a, double b) { return k == 0 ? fmin(a, b) : fmax(a, b); }
  static __host__ __device__ double empty(int k) { return k == 0 ? 1e300 : -1e300; }
};
struct AbsMaxRule {              // the maximum of non-negative values; a NaN on either side stays a NaN
  static __host__ __device__ double combine(int, double a, double b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }
  static __host__ __device__ double empty(int) { return 0.; }
};

// ---- the site of a thread: a 256-thread block over the padded plane, grid (plane blocks, planes from p0) -------------
struct PlaneSite { long long s; int x, y, p, z; bool in; };   // offset in the plane, storage plane p, global z, inside the lattice
__device__ __forceinline__ PlaneSite plane_site(const Geo& G, int p0) {
  PlaneSite st;
  st.s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  st.p = p0 + (int)blockIdx.y;
  st.y = (int)(st.s / G.pitch);
  st.x = (int)(st.s - (long long)st.y * G.pitch);
  st.z = G.z0 + (st.p - G.H);
  st.in = st.s < G.plane && st.x < G.nx;
  return st;
}

// ---- the workgroup tree over NV values: a[t] = combine(a[t], a[t + w]), w = 128 .. 1; the results are sh[k][0] -------
typedef double Column[256];
template <int NV, class Rule>
__device__ __forceinline__ const Column* block_tree(const double (&v)[NV]) {
  __shared__ double sh[NV][256];
  for (int k = 0; k < NV; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) for (int k = 0; k < NV; ++k) sh[k][threadIdx.x] = Rule::combine(k, sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
    __syncthreads();
  }
  return sh;
}

// the tail of stage 1: the tree, then thread 0 writes the block's partial
template <int NV, class Rule = SumRule>
__device__ __forceinline__ void block_reduce(const double (&v)[NV], double* __restrict__ partial) {
  const Column* sh = block_tree<NV, Rule>(v);
  if (threadIdx.x == 0) {
    const long long b = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    for (int k = 0; k < NV; ++k) partial[b * NV + k] = sh[k][0];
  }
}

// stage 2 of one plane: all nbx block partials of the plane (fixed order: every thread a 256-strided subsequence, then
// the tree).  A thread reads only its own column of the result before the next call's barrier.
template <int NV, class Rule>
__device__ __forceinline__ const Column* plane_reduce(const double* __restrict__ partial, int nbx) {
  double v[NV];
  for (int k = 0; k < NV; ++k) v[k] = Rule::empty(k);
  for (int b = threadIdx.x; b < nbx; b += 256) for (int k = 0; k < NV; ++k) v[k] = Rule::combine(k, v[k], partial[(long long)b * NV + k]);
  return block_tree<NV, Rule>(v);
}
// one workgroup per plane, so that a reduction hands O(nz) doubles to the host instead of one per block -- the
// gradient-flow fit runs ~400 such reductions per fit, at 512^3 that was 8 MB per reduction
template <int NV, class Rule>
__global__ void __launch_bounds__(256) k_plane_partials(const double* __restrict__ partial, double* __restrict__ out, int nbx) {
  const Column* sh = plane_reduce<NV, Rule>(partial + (long long)blockIdx.x * nbx * NV, nbx);
  if (threadIdx.x == 0) for (int k = 0; k < NV; ++k) out[(long long)blockIdx.x * NV + k] = sh[k][0];
}

// ---- one reduction of a slab's own planes -----------------------------------------------------------------------------
// launch(grid, partial) enqueues stage 1 on c->stream; the results are COMBINED INTO `out`, which the caller initialised.
//   Fold::HostBlocks  every block partial is copied and combined on the host in block order (scratch: c->partial, 5
//                     doubles per block): mass, com_sums, update_com, prepare_ref, the absmax of an upload.
//   Fold::Planes      stage 2 on the device, the planes combined on the host in sequence (scratch: the idle state buffer,
//                     far larger than (blocks + planes) * NV).  A caller that passes the slabs of a ring in order runs
//                     over the planes of the whole lattice in one fixed sequence whatever the decomposition: the ring
//                     gives the same doubles as the single context.
// resident: rho / phi are to hold the densities of the resident state (refused inside an open step); false: the caller
// has enqueued its own density pass.
enum class Fold { HostBlocks, Planes };
template <int NV, class Rule, class Launch>
int slab_reduce(bflbm_ctx* c, Fold fold, bool resident, double (&out)[NV], Launch launch) {
  static_assert(NV <= 20, "scratch sizing");
  if (resident && c->step_open()) return fail("reduction requested inside an open step");
  HIP_TRY(hipSetDevice(c->dom.device));
  if (resident && ensure_density(c)) return 1;
  const dim3 g = plane_grid(c, c->nzl);
  size_t n = (size_t)g.x * g.y;
  double* scratch = fold == Fold::Planes ? c->S[1 - c->cur] : c->partial;
  launch(g, scratch);
  HIP_TRY(hipGetLastError());
  if (fold == Fold::Planes) {
    double* planes = scratch + n * NV;
    hipLaunchKernelGGL((k_plane_partials<NV, Rule>), dim3(g.y), dim3(256), 0, c->stream, scratch, planes, (int)g.x);
    HIP_TRY(hipGetLastError());
    scratch = planes; n = g.y;
  }
  std::vector<double> h(n * NV);
  HIP_TRY(hipMemcpyAsync(h.data(), scratch, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t b = 0; b < n; ++b) for (int k = 0; k < NV; ++k) out[k] = Rule::combine(k, out[k], h[b * NV + k]);
  return 0;
}

}  // namespace

// ---- the slab reductions of the core (deterministic: per-block partials, combined on the host in block order)
// out[b][0..5] = sum rho, sum phi, sum rho*i, sum rho*j, sum rho*k (global k)
__global__ void __launch_bounds__(256) k_reduce(const double* __restrict__ rho, const double* __restrict__ phi,
                                                double* __restrict__ partial, Geo G, int p0) {
  const PlaneSite st = plane_site(G, p0);
  double v[5] = {0., 0., 0., 0., 0.};
  if (st.in) {
    const long long o = (long long)st.p*G.plane + st.s;
    const double r = rho[o];
    v[0] = r; v[1] = phi[o]; v[2] = r*st.x; v[3] = r*st.y; v[4] = r*st.z;
  }
  block_reduce<5>(v, partial);
}

// largest |rho + phi| per block over the slab's own planes (what `auto` keys its stability bound on after an upload,
// bflbm_commit_upload); NaN propagates to the result so that a broken upload is not mistaken for a small one
__global__ void __launch_bounds__(256) k_total_absmax(const double* __restrict__ rho, const double* __restrict__ phi,
                                                      double* __restrict__ partial, Geo G, int p0) {
  const PlaneSite st = plane_site(G, p0);
  double v[1] = {0.};
  if (st.in) {
    const long long o = (long long)st.p*G.plane + st.s;
    v[0] = fabs(rho[o] + phi[o]);
  }
  block_reduce<1, AbsMaxRule>(v, partial);
}

#endif  // BFLBM_REDUCE_H_
