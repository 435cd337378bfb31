// bflbm_fused.h -- fused plane-marching collide-and-stream kernel (schedule 1).
//
// One HBM pass per LBM_timestep: read 38 populations, write 38 populations per site.
//
// Each workgroup owns a TX x TY tile in (x,y) and marches through a chunk of planes along z.
// At march position q every thread
//   1. pulls the 38 populations of its site in plane q (f_i(x) = S_i(x - c_i), coalesced along x)
//      and keeps them in registers;
//   2. sums them in the reference's order -> rho,phi of plane q (LBM_binary.H:320-330) into an
//      LDS ring slot; the lanes of the tile additionally pull-and-sum the one-site ring around
//      the tile (those loads are L2 hits: the neighbouring tile's workgroup streams the same
//      lines), so the slot covers (TX+2) x (TY+2) sites;
//   3. after one barrier, collides plane q-1 from the registers kept at the previous position,
//      with the 18-neighbour gradient stencil (LBM_binary.H:134-150) served from the LDS slots
//      of planes q-2, q-1, q, and writes the post-collision populations of plane q-1.
// The slab is split into chunks of planes so that the grid has >> 256 workgroups; a chunk of
// L planes pulls L+2 planes (the two extra only for their densities).
//
// The arithmetic is the same device functions as the two-pass schedule (bflbm_site.h), so both
// schedules and the CPU oracle agree bit for bit.
#ifndef BFLBM_FUSED_H_
#define BFLBM_FUSED_H_

#include <type_traits>
#include "bflbm_kernels.h"

struct FusedGrid {
  int ntx, nty;        // tiles in x and y
  int pa, pb;          // storage planes [pa,pb) to advance
  int lz;              // planes per chunk
  int cstride;         // planes between the starts of consecutive chunks (== lz unless the chunks are disjoint)
  int nchunks;
  int ncols;           // ntx*nty
  int total;           // ncols*nchunks workgroups
  int per_xcd;         // ceil(total/8)
  int sx;              // strip width (tiles in x) of the column order, see fused_map
  int row0 = 0;        // the column order starts at this tile row (hand-over kernel on a lattice with a lower last tile row)
};

// Workgroup -> (column, chunk).  Workgroups b and b+8 share an XCD (round-robin dispatch), so give
// each XCD a contiguous band of tile columns: halo lines are then shared through that XCD's L2.
// Placement only affects speed.
__device__ __forceinline__ void fused_col(const FusedGrid& F, int w, int& col, int& chunk);
__device__ __forceinline__ bool fused_map(const FusedGrid& F, int b, int& col, int& chunk) {
  const int xcd = b & 7, j = b >> 3;
  const int w = xcd * F.per_xcd + j;             // position in the XCD-major work list
  if (j >= F.per_xcd || w >= F.total) return false;
  fused_col(F, w, col, chunk);
  return true;
}
// position w of one lattice's work list -> (tile column, chunk)
__device__ __forceinline__ void fused_col(const FusedGrid& F, int w, int& col, int& chunk) {
  // inside the list: chunk-major over groups of columns so that concurrently resident workgroups
  // of one XCD are neighbouring columns of the same chunk
  chunk = w / F.ncols;
  const int c = w % F.ncols;
  // column order inside the list: strips of F.sx tiles in x, tile rows (y) fastest inside a strip, so that the
  // workgroups resident together on an XCD cover a compact block whose inner ring rows are shared through L2
  // (sx == ntx is row-major order: a band of whole tile rows)
  if (F.sx >= F.ntx) { col = c; }
  else {
    const int per_strip = F.sx * F.nty;
    const int strip = c / per_strip, r = c - strip * per_strip;
    const int w_strip = min(F.sx, F.ntx - strip * F.sx);       // last strip may be narrower
    const int tiy = r / w_strip, tix = strip * F.sx + (r - tiy * w_strip);
    col = tiy * F.ntx + tix;
  }
}


// Tile geometry: TX x TY threads, one site each, tiles aligned to TX (row segments start on
// 128-byte lines when TX is a multiple of 16).  rho,phi of the one-site ring around the tile are
// pulled and summed as 2*ring half-tasks (site x fluid) spread evenly over the waves.
template <int TX, int TY, int MODE>   // MODE 0: no noise, 1: generated noise, 2: injected noise
__global__ void __launch_bounds__(TX*TY, 2)
k_fused(const double* __restrict__ S, double* __restrict__ D,
        const double* __restrict__ injf, const double* __restrict__ injg,
        Geo G, DevParams P, FusedGrid F, uint32_t noise_index) {
  constexpr bool UNIT = false;
#define BFLBM_FUSED_MAP(col, chunk) fused_map(F, (int)blockIdx.x, col, chunk)
#include "bflbm_fused_body.inc"
#undef BFLBM_FUSED_MAP
}
// zero noise at unit relaxation rates (unit_rates(P)): the same source with d_relax_with's unit-rate form, under its own
// name so that k_fused's symbols and code stay what they were
template <int TX, int TY>
__global__ void __launch_bounds__(TX*TY, 2)
k_fused_unit(const double* __restrict__ S, double* __restrict__ D,
             const double* __restrict__ injf, const double* __restrict__ injg,
             Geo G, DevParams P, FusedGrid F, uint32_t noise_index) {
  constexpr int MODE = 0;
  constexpr bool UNIT = true;
#define BFLBM_FUSED_MAP(col, chunk) fused_map(F, (int)blockIdx.x, col, chunk)
#include "bflbm_fused_body.inc"
#undef BFLBM_FUSED_MAP
}

constexpr int FUSED_TX = 64, FUSED_TY = 8;   // tile shape of the fused kernel (narrower lattices at zero noise: see launch_plan)
constexpr int HO_TY = 4;                     // tile height of the hand-over kernel of bflbm_handover.h (tiles are 64 x HO_TY)

// ---- the launch-plan layer: host arithmetic, no ambient state.  ncu is the compute-unit count of the device of whoever
// launches: a context's own (bflbm_ctx::ncu), a batch's replicas', or what a plan query was given.
// The cut of one step over a context's own storage planes [lo, hi) = [H, H + nzl).  A periodic lattice is all interior
// (pair_len 0).  A slab advances its two boundary pairs of pair_len = 2 planes, [lo, a) and [b, hi), first
// (bflbm_step_boundary: its neighbours wait for them) and the interior [a, b) while they travel (bflbm_step_interior); a slab
// of 4 planes has no interior (b <= a).  one_pair_launch: the pairs are disjoint and the plane-marching kernels take both in
// ONE launch over [lo, hi).
struct StepRanges { int lo, hi, pair_len, a, b; bool one_pair_launch; };
static inline StepRanges step_ranges(const Geo& G, int nzl) {
  const int lo = G.H, hi = G.H + nzl, pair_len = G.zwrap ? 0 : 2;
  return {lo, hi, pair_len, lo + pair_len, hi - pair_len, pair_len > 0 && hi - lo > 2 * pair_len};
}

// Chunking of a launch of np planes over F.ncols tile columns (both plane-marching kernels); fills lz, nchunks, cstride,
// total and per_xcd.  min_chunk: the shortest chunk the kernel takes.  nrep > 1: a replica batch launches nrep copies of
// the plan (bflbm_batch.h), so the search counts all of their workgroups.  pair_len > 0: ONE launch over the two disjoint
// plane ranges [pa, pa+pair_len) and [pb-pair_len, pb) (the boundary plane pairs of a slab), one chunk each.
//
// One workgroup is resident per CU, so the launch runs in rounds of `ncu` workgroups and costs about
// rounds x (planes per chunk + 1) plane marches (a chunk of L planes marches L+2, the two extra ones pull only).  Pick the
// chunk count that minimises this: 256^3 -> 128 columns x 2 chunks = one full round; 192^3 -> 72 columns x 7 chunks = 504
// workgroups in 2 rounds of 30 planes instead of 288 in "1.1" rounds of 50.  Marches longer than 256 planes are avoided on
// a single slab (neighbouring workgroups drift apart and lose L2 sharing; measured on MI355X, and one 512-plane march per
// column of the hand-over kernel was A/B-tested: -1 %); a slab of a multi-GPU run is cut into >= 3 rounds of shorter
// workgroups so that the RCCL copy kernels of the overlapped exchange, which need a few CUs of their own, delay at most a
// short tail of the interior sweep.  Round 4 scanned the hand-over kernel's chunk count at 256^3 ... 512^3 on two boxes
// (profiles/r04_chunk_scan.txt): a model fitted on the first box ((rounds + tail) x (planes + 4): 448^3 +5 % with 7
// chunks, 512^3 +5 % with 4) changed nothing on the second (every lattice within the +-2 % process-to-process scatter,
// 512x512x128 2 % SLOWER with its choice), so the rule stays.
static inline void plan_chunks(FusedGrid& F, int np, bool zwrap, int min_chunk, int nrep, int pair_len, int ncu) {
  constexpr int min_slab_rounds = 3;
  const int maxchunks = std::max(1, np / min_chunk);             // small lattices: short chunks buy parallelism
  long long best = -1;
  int nchunks = 1;
  for (int k = 1; k <= maxchunks; ++k) {
    const int lz = (np + k - 1) / k, chunks = (np + lz - 1) / lz;
    if (chunks != k) continue;                                    // same partition as a smaller k
    if (zwrap && lz > 256 && k < maxchunks) continue;
    const long long total = (long long)F.ncols * chunks * nrep, rounds = (total + ncu - 1) / ncu;
    if (!zwrap && rounds < min_slab_rounds && k < maxchunks) continue;
    const long long cost = rounds * (lz + 1);
    if (best < 0 || cost < best) { best = cost; nchunks = k; }
  }
  F.lz = (np + nchunks - 1) / nchunks;
  F.nchunks = (np + F.lz - 1) / F.lz;
  F.cstride = F.lz;
  if (pair_len > 0 && np > 2 * pair_len) { F.lz = pair_len; F.nchunks = 2; F.cstride = np - pair_len; }
  F.total = F.ncols * F.nchunks;
  F.per_xcd = (F.total + 7) / 8;
}

// The plan of one launch of schedule sch (3: the hand-over kernel of bflbm_handover.h; otherwise the fused kernel) over the
// storage planes [pa, pb): fills F with tiles, chunking and workgroup order and returns the tile width (the height is threads /
// width).  The hand-over form returns 64 (tiles of 64 x HO_TY) and ignores mode and threads.  nrep, pair_len: see plan_chunks.
// threads: workgroup size of the fused kernel (tiles of at least 8 rows; the batch's noise kernel runs 256)
static inline int launch_plan(int sch, const Geo& G, int pa, int pb, int pair_len, int mode, int ncu, FusedGrid& F, int nrep = 1,
                              int threads = FUSED_TX * FUSED_TY) {
  const bool ho = sch == 3;
  // Tile shape of the fused kernel: 64 x 8 sites; lattices narrower than 64 in x get the same 512 sites as 32 x 16, 16 x 32 or
  // 8 x 64 (zero noise only; e.g. the reference's 8 x 256 x 64 flat-interface box would use 8 of 64 lanes of a 64-wide tile)
  const int TX = ho ? 64 : std::min((mode != 0 || G.nx > 32) ? FUSED_TX : (G.nx > 16 ? 32 : (G.nx > 8 ? 16 : 8)), threads / 8);
  const int TY = ho ? HO_TY : threads / TX;
  F.ntx = (G.nx + TX - 1) / TX;
  F.nty = (G.ny + TY - 1) / TY;
  F.ncols = F.ntx * F.nty;
  F.pa = pa; F.pb = pb;
  plan_chunks(F, pb - pa, G.zwrap, ho ? 4 : 2, nrep, pair_len, ncu);   // a hand-over chunk shorter than 4 planes has no complete frame
  F.sx = ho ? F.ntx : std::min(F.ntx, 4);      // fused: strips of 4 tiles: +2 % at 512^3 (ntx = 8), identical at 256^3
  return TX;
}

// launch(std::integral_constant<int, TX>()) for the tile width TX of a zero-noise plan of the fused kernel, one of
// 64, 32, 16, 8 (the height is FUSED_TX * FUSED_TY / TX): how a launch picks the kernel's tile instantiation
template <class Launch> void fused_dispatch_tile(int TX, Launch&& launch) {
  if (TX == 32)      launch(std::integral_constant<int, 32>());
  else if (TX == 16) launch(std::integral_constant<int, 16>());
  else if (TX == 8)  launch(std::integral_constant<int, 8>());
  else               launch(std::integral_constant<int, FUSED_TX>());
}

// returns the launch's error code
static inline hipError_t fused_launch(const double* S, double* D, const double* injf, const double* injg,
                               const Geo& G, const DevParams& P, int pa, int pb,
                               uint32_t noise_index, int mode, int ncu, hipStream_t stream, int pair_len = 0) {
  FusedGrid F;
  const int TX = launch_plan(1, G, pa, pb, pair_len, mode, ncu, F);
  dim3 grid((unsigned)(F.per_xcd * 8)), block(FUSED_TX * FUSED_TY);
  if (mode == 2)      hipLaunchKernelGGL((k_fused<FUSED_TX, FUSED_TY, 2>), grid, block, 0, stream, S, D, injf, injg, G, P, F, noise_index);
  else if (mode == 1) hipLaunchKernelGGL((k_fused<FUSED_TX, FUSED_TY, 1>), grid, block, 0, stream, S, D, injf, injg, G, P, F, noise_index);
  else fused_dispatch_tile(TX, [&](auto tx) {
    constexpr int X = decltype(tx)::value, Y = (FUSED_TX * FUSED_TY) / X;
    if (unit_rates(P)) hipLaunchKernelGGL((k_fused_unit<X, Y>), grid, block, 0, stream, S, D, injf, injg, G, P, F, noise_index);
    else               hipLaunchKernelGGL((k_fused<X, Y, 0>), grid, block, 0, stream, S, D, injf, injg, G, P, F, noise_index);
  });
  return hipGetLastError();
}

#endif  // BFLBM_FUSED_H_
