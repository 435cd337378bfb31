// bflbm_batch.h -- replica batches: B independent periodic lattices of one shape advanced by one launch per pass.
//
// The replica is part of the grid (two-pass: blockIdx.z; fused: a replica-major fold of the workgroup list), and
// everything that differs between replicas -- model parameters, the two state buffers, rho/phi, the noise index --
// comes from a per-replica record in device memory, read with uniform (scalar) loads: nothing per replica is a kernel
// argument, so B may be in the hundreds.  The records are written by the host only when a replica changed; between
// uploads the kernels derive the current buffer and noise index from `k`, the batch steps since the upload.
// The arithmetic is the single-lattice kernels' own source (bflbm_collide_body.inc, bflbm_fused_body.inc and the device
// functions of bflbm_site.h), so every replica computes the doubles a lone lattice computes.
#ifndef BFLBM_BATCH_H_
#define BFLBM_BATCH_H_

#include "bflbm_fused.h"

struct BatchRec {
  DevParams P;
  double* S[2];        // the replica's two state buffers
  double* rho;
  double* phi;
  uint32_t idx0;       // noise index (step counter) of the replica when the record was written
  int cur0;            // its resident buffer then
};

// the record of replica r in the constant address space: loads from it are scalar wherever the index is uniform
typedef const __attribute__((address_space(4))) BatchRec* BatchRecC;
__device__ __forceinline__ BatchRecC batch_rec(const BatchRec* recs, int r) { return (BatchRecC)(recs + r); }
__device__ __forceinline__ const DevParams& batch_params(BatchRecC R) { return *(const DevParams*)&R->P; }

// The per-replica bodies take the replica's pointers as __restrict__ parameters (what the single-lattice kernels get from
// their argument list) and compile the single-lattice kernels' own source text.

// pass A, grid (plane blocks, nz, B): rho,phi of the streamed state (k_density)
__device__ __forceinline__ void density_batch_body(const double* __restrict__ S, double* __restrict__ rho,
                                                   double* __restrict__ phi, const Geo& G, int p0) {
  BFLBM_SITE_FROM_BLOCK();
  SiteOff I; site_offsets(G, x, y, p, I);
  double fs[Q], gs[Q];
  pull_site(S, G, I, fs, gs);
  st_sb(rho + I.pl[1], I.o[1][1], d_density(fs));
  st_sb(phi + I.pl[1], I.o[1][1], d_density(gs));
}
__global__ void __launch_bounds__(256) k_density_batch(const BatchRec* __restrict__ recs, Geo G, int k) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  density_batch_body(R->S[cur], R->rho, R->phi, G, 0);
}

// pass B, grid (plane blocks, nz, B): k_collide without injected noise and reference state
template <bool NOISE, bool UNIT>
__device__ __forceinline__ void collide_batch_body(const double* __restrict__ S, double* __restrict__ D,
                                                   const double* __restrict__ rho, const double* __restrict__ phi,
                                                   const Geo& G, const DevParams& P, uint32_t noise_index) {
  constexpr bool INJECT = false;
  const double* __restrict__ injf = nullptr;
  const double* __restrict__ injg = nullptr;
  const int p0 = 0;
  RefState Rf;
  Rf.rho = Rf.phi = Rf.rhot = nullptr;
  Rf.on = 0; Rf.sx = Rf.sy = Rf.sz = 0;
#include "bflbm_collide_body.inc"
}
template <bool NOISE>
__global__ void __launch_bounds__(256, COLLIDE_WAVES) k_collide_batch(const BatchRec* __restrict__ recs, Geo G, int k) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  collide_batch_body<NOISE, false>(R->S[cur], R->S[cur ^ 1], R->rho, R->phi, G, batch_params(R), R->idx0 + (uint32_t)k);
}

// zero noise with every replica at unit relaxation rates (unit_rates): d_relax_with's unit-rate form
__global__ void __launch_bounds__(256, COLLIDE_WAVES) k_collide_batch_unit(const BatchRec* __restrict__ recs, Geo G, int k) {
  const BatchRecC R = batch_rec(recs, (int)blockIdx.z);
  const int cur = R->cur0 ^ (k & 1);
  collide_batch_body<false, true>(R->S[cur], R->S[cur ^ 1], R->rho, R->phi, G, batch_params(R), R->idx0 + (uint32_t)k);
}

// one-pass schedule: nrep * F.total workgroups.  Workgroups b and b+8 share an XCD (round-robin dispatch); the work list
// is split into 8 contiguous parts, replica-major, so that an XCD holds whole replicas (a replica's ring lines stay in one
// L2).  Returns the replica r and the position w in its own work list (fused_col).
__device__ __forceinline__ bool batch_map(const FusedGrid& F, int nrep, int b, int& r, int& w) {
  const int per_xcd = (nrep * F.total + 7) / 8;
  const int xcd = b & 7, j = b >> 3;
  const int wg = xcd * per_xcd + j;
  if (j >= per_xcd || wg >= nrep * F.total) return false;
  r = wg / F.total;
  w = wg - r * F.total;
  return true;
}

template <int TX, int TY, int MODE, bool UNIT>
__device__ __forceinline__ void fused_batch_body(const double* __restrict__ S, double* __restrict__ D,
                                                 const Geo& G, const DevParams& P, const FusedGrid& F, uint32_t noise_index, int w) {
  const double* __restrict__ injf = nullptr;
  const double* __restrict__ injg = nullptr;
#define BFLBM_FUSED_MAP(col, chunk) (fused_col(F, w, col, chunk), true)
#include "bflbm_fused_body.inc"
#undef BFLBM_FUSED_MAP
}
// MODE 1 runs 32 x 8 tiles at one wave per SIMD: the noise body needs more than the 256 registers a 512-thread workgroup
// leaves a wave (the single-lattice k_fused<64, 8, 1> spills to scratch)
template <int TX, int TY, int MODE>
__global__ void __launch_bounds__(TX*TY, MODE == 1 ? 1 : 2)
k_fused_batch(const BatchRec* __restrict__ recs, Geo G, FusedGrid F, int nrep, int k) {
  int r, w;
  if (!batch_map(F, nrep, (int)blockIdx.x, r, w)) return;   // whole workgroup leaves together
  const BatchRecC R = batch_rec(recs, r);
  const int cur = R->cur0 ^ (k & 1);
  fused_batch_body<TX, TY, MODE, false>(R->S[cur], R->S[cur ^ 1], G, batch_params(R), F, R->idx0 + (uint32_t)k, w);
}

// zero noise with every replica at unit relaxation rates (unit_rates): d_relax_with's unit-rate form
template <int TX, int TY>
__global__ void __launch_bounds__(TX*TY, 2)
k_fused_batch_unit(const BatchRec* __restrict__ recs, Geo G, FusedGrid F, int nrep, int k) {
  int r, w;
  if (!batch_map(F, nrep, (int)blockIdx.x, r, w)) return;   // whole workgroup leaves together
  const BatchRecC R = batch_rec(recs, r);
  const int cur = R->cur0 ^ (k & 1);
  fused_batch_body<TX, TY, 0, true>(R->S[cur], R->S[cur ^ 1], G, batch_params(R), F, R->idx0 + (uint32_t)k, w);
}

// the batch's tile shape and chunking: the single-lattice plan with the workgroups of all replicas counted
static inline int batch_fused_threads(int mode) { return mode == 1 ? 256 : FUSED_TX * FUSED_TY; }
static inline int batch_fused_plan(const Geo& G, int nrep, int mode, int ncu, FusedGrid& F) {
  return launch_plan(1, G, 0, G.nzs, 0, mode, ncu, F, nrep, batch_fused_threads(mode));
}

// unit: the caller found zero noise and unit_rates() in every replica
static inline hipError_t batch_fused_launch(const BatchRec* recs, const Geo& G, int nrep, int mode, bool unit, int k, int ncu, hipStream_t stream) {
  FusedGrid F;
  const int TX = batch_fused_plan(G, nrep, mode, ncu, F);
  const long long per_xcd = ((long long)nrep * F.total + 7) / 8;
  if (per_xcd * 8 > (long long)INT32_MAX) return hipErrorInvalidConfiguration;
  dim3 grid((unsigned)(per_xcd * 8)), block(batch_fused_threads(mode));
  if (mode == 1) hipLaunchKernelGGL((k_fused_batch<32, 8, 1>), grid, block, 0, stream, recs, G, F, nrep, k);
  else fused_dispatch_tile(TX, [&](auto tx) {
    constexpr int X = decltype(tx)::value, Y = (FUSED_TX * FUSED_TY) / X;
    if (unit) hipLaunchKernelGGL((k_fused_batch_unit<X, Y>), grid, block, 0, stream, recs, G, F, nrep, k);
    else      hipLaunchKernelGGL((k_fused_batch<X, Y, 0>), grid, block, 0, stream, recs, G, F, nrep, k);
  });
  return hipGetLastError();
}

static inline hipError_t batch_two_pass_launch(const BatchRec* recs, const Geo& G, int nrep, bool noise, bool unit, int k, hipStream_t stream) {
  const dim3 grid((unsigned)((G.plane + 255) / 256), (unsigned)G.nzs, (unsigned)nrep), block(256);
  hipLaunchKernelGGL(k_density_batch, grid, block, 0, stream, recs, G, k);
  if (noise) hipLaunchKernelGGL((k_collide_batch<true>), grid, block, 0, stream, recs, G, k);
  else if (unit) hipLaunchKernelGGL(k_collide_batch_unit, grid, block, 0, stream, recs, G, k);
  else       hipLaunchKernelGGL((k_collide_batch<false>), grid, block, 0, stream, recs, G, k);
  return hipGetLastError();
}

#endif  // BFLBM_BATCH_H_
