// bflbm_handover.h -- fused plane-marching collide-and-stream kernel with a cross-step hand-over of the
// tile-boundary densities (schedule 3).
//
// The plane march of bflbm_fused.h needs rho,phi of the streamed state on a one-site ring around each
// workgroup's tile (gradient stencil, LBM_binary.H:134-150 applied to the densities of :315-330).  There
// the ring is pulled: 19 loads per ring site and fluid to produce one number, lines that belong to the
// neighbouring tiles (measured: 1.33x-1.6x the algorithmic read bytes, profiles/r01_*).  Here the ring
// densities of step t+1 are handed over from step t instead:
//
//   rho_{t+1}(r) = sum_i f*_i(r - c_i)           (f* = post-collision populations of step t)
//
// While the 19 outputs of a site are in registers the producing workgroup sorts them by destination:
//   x  wave shifts (DPP wave_shr/wave_shl, a tile row is one 64-lane wave)       -> 9 buckets (dy,dz)
//   z  a two-stage register/LDS pipeline along the march                          -> 3 sums (dy)
//   y  finished sums of the row next to an edge row cross through LDS
// and writes per tile, plane and fluid a FRAME of partial sums over the sources INSIDE the tile:
//   E  for its own edge sites      (2*64 + 2*(TY-2) values)   -- what the neighbours are missing
//   O  for the ring sites outside  (2*64 + 2*(TY+2) values)   -- what it contributes to the neighbours
// Step t+1 forms the ring density of a site as  E(owner tile) + O(own tile) [+ O of the two other tiles
// at the 12 sites next to a tile corner]: 2-4 loads instead of 19.  Frame traffic: 2*FR/(64*TY) values per
// site and fluid each way (64x4 tiles: +5.7 % of 608 B/site).
//
// The tile's OWN densities are still summed from the pulled populations in the reference's order.  The ring
// densities are sums of the same 19 numbers in a different, fixed order: deterministic, equal to the
// reference's to an ulp, not bit-identical; they only enter the gradient of the tile's edge sites.  The
// schedule is therefore held to the north-star tolerance (rho,phi rel 1e-12, u abs 1e-12 cs) and the two
// bit-exact schedules (0 two-pass, 1 fused with pulled ring) remain the cross-check.
//
// Frames of the first and last plane of a chunk would need sources of the neighbouring chunk: those planes
// (and every plane of the first step after an init/upload) use the pulled ring.
//
// Lattices that are not whole tiles (template flag RAG; the full-tile kernel is compiled without any of it):
//   x  the last tile of a row may be narrower (aw < 64 sites): its idle lanes load a duplicate of the last site, store
//      nothing and contribute zeros to the x shifts; its right column lane is aw-1 and its right ring column aw+1, and
//      the frames keep their layout (slots are roles, not coordinates), so a narrow tile hands over like any other.
//   y  the last tile row may be lower (ah < TY rows).  In a full tile every row has ONE y role (bottom edge, hands its -y
//      sum down, hands its +y sum up, top edge); in a tile of 2 or 3 rows a row has two (ah = 2: row 0 is the bottom
//      edge AND hands its +y sum to row 1), so the ragged kernel runs both travelling sums in every row and picks by
//      role; the frame keeps its layout with the top row / top ring row at ah-1 / ah.  (ah = 1, like aw = 1, is
//      refused by the host: a ring site owned by such a tile also collects from the tile beyond it.)
// A ring site is looked up by its coordinates RELATIVE to each of the 3 x 3 surrounding tiles (not by wrapped global
// coordinates), so a lattice one tile wide or high -- where the neighbour on both sides is the tile itself and a ring
// site is one of its own edge sites at the same time -- needs nothing special: nx >= 64 (one tile: nx = 64), ny >= TY.
#ifndef BFLBM_HANDOVER_H_
#define BFLBM_HANDOVER_H_

#include "bflbm_fused.h"

// Requests of the next plane's f half in the steady state: one every HO_SPREAD_F VALU instructions of the relaxation of
// fluid f instead of one burst of 19 before it (see the comment at the call site).  The noise kernel, round 4: with the
// 11-instruction normals one request every 44 VALU instructions is +2.3 % at 512^3 and +2.0 % at 256^3 (16 ... 32: -1 %,
// 56: 0, 68: +2.5 / +0.5 %); round 3's generator: every spacing lost.
constexpr int HO_SPREAD_F = 28;      // quiet kernel
constexpr int HO_SPREAD_F1 = 44;     // noise kernel
// The unit-rate quiet kernels (k_fused_ho_unit): their block of gradient, projection and relaxation of f is about 110 VALU
// instructions shorter.  Full tiles: at 28 the kernel measures what the generic one measures (8547 against 8543 MLUPS at
// 512^3).  Scanned on two boxes, 2-3 interleaved processes each agreeing to 0.1 % (profiles/unit_rate_spacing.txt), relative to
// the generic kernel on the same box, 512^3 / 256^3: 20 -3.6 / -4.0 %, 24 -0.4 / -0.3, 26 -5.5 / -4.8, 28 0 / -0.3, 30 +0.3 / +0.4
// and +0.3 / -0.2, 31 +1.2 / -0.4, 32 +1.3 / -0.1 and +1.4 / -0.2, 33 +2.2 / +0.9, 34 +1.3 / -0.2, 36 +1.0 / -1.3, 40 +1.0 / 0.
// At 33 the solver places 14 single requests (one gap of 66) and leaves the last five next to the f stores: an optimum found
// by measurement, which another compiler may move.  Ragged tiles: only 28 and 33 were measured (500^3 / 250^3, three
// processes each): 28 +3.3 / +1.8 %, 33 +2.7 / +1.4 % against the generic ragged kernel, so that instantiation keeps 28.
constexpr int HO_SPREAD_FU = 33;       // full tiles
constexpr int HO_SPREAD_FU_RAG = 28;   // ragged tiles
// Outputs of fluid g that the full-tile unit-rate kernel stores one march position later (see the stores in front of the barrier in
// bflbm_handover_body.inc).  The last four that finish_fluid forms (11..14, the yz diagonals) are stored at once: they are
// younger than the last request of the g half, so the waits at the loop head stay vmcnt(4) and above and cover loads only
// (with none kept the head ended in vmcnt(0) on the row's frame store).  512^3, MLUPS against the parent's 8745-8773 on the
// same box: kept 1: 8935, 2: 9019-9030, 3: 9054, 4: 9037, 6: 8998, 9: 8953.
constexpr bool ho_g_deferred(int i) { return i < 11 || i > 14; }

template <int TY> struct HoLayout {
  static constexpr int TX = 64;
  // slots of one fluid's frame (doubles): the four 64-entry rows first, each on its own 128-byte lines (they are stored
  // and loaded by whole waves), the column entries (4*TY doubles, one line for TY = 4) behind them
  static constexpr int EB = 0, ET = TX, OB = 2 * TX, OT = 3 * TX;
  static constexpr int EL = 4 * TX, ER = EL + (TY - 2), OL = ER + (TY - 2), OR_ = OL + (TY + 2);
  static constexpr int FR = OR_ + (TY + 2);            // 4*TX + 4*TY: 272 (TY=4), 288 (TY=8) -- whole 128-byte lines
  static constexpr int REC = 2 * FR;                   // both fluids
};

struct HoGrid {
  const double* fin;     // frames of the state being read   [plane][tile][fluid][FR]
  double* fout;          // frames of the state being written
  long long fplane;      // doubles per plane = ntiles * REC
  int use_frames;        // fin holds frames written by the same launch geometry one step earlier
};

// destination slot of lattice site (lx,ly), given relative to a tile's origin, in that tile's frame; -1: none
template <int TYL>
__device__ __forceinline__ int ho_frame_slot(int lx, int ly, int TX /* width */, int TY /* height of the tile that owns the frame */) {
  using L = HoLayout<TYL>;
  if (lx >= 0 && lx < TX && ly >= 0 && ly < TY) {
    if (ly == 0) return L::EB + lx;
    if (ly == TY - 1) return L::ET + lx;
    if (lx == 0) return L::EL + ly - 1;
    if (lx == TX - 1) return L::ER + ly - 1;
    return -1;
  }
  if (lx >= 0 && lx < TX) {
    if (ly == -1) return L::OB + lx;
    if (ly == TY) return L::OT + lx;
    return -1;
  }
  if (ly >= -1 && ly <= TY) {
    if (lx == -1) return L::OL + ly + 1;
    if (lx == TX) return L::OR_ + ly + 1;
  }
  return -1;
}
__device__ __forceinline__ double ho_shr(double v) {   // value of lane-1 (travelling +x), 0 in lane 0
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double ho_shl(double v) {   // value of lane+1 (travelling -x), 0 in lane 63
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// ONE workgroup per CU at one wave per SIMD (512 registers per lane, AGPRs included, 160 KB of LDS): the pending
// plane of BOTH fluids waits in LDS, and the loads of plane q+1 are issued before plane q-1 is collided -- the f half
// before fluid f is relaxed, the g half after it is finished -- so that memory latency runs under the arithmetic
// inside one wave instead of between waves.  (At two waves per SIMD the frame producer spills 59-90 registers; that
// form, and the variants that kept the f plane in registers or requested the next plane before the density sums,
// were measured and removed: NOTES.md section 3.1b.)
// MODE 0: zero noise; MODE 1: generated thermal noise (csrc/bflbm_rng.h), drawn where it is added.
// RAG: the lattice has a narrower last tile column and/or a lower last tile row (see the header comment)
template <int TY, int MODE, bool RAG>
__global__ void __launch_bounds__(64 * TY, 1)
k_fused_ho(const double* __restrict__ S, double* __restrict__ D, Geo G, DevParams P, FusedGrid F, HoGrid Hg, uint32_t noise_index) {
  constexpr bool UNIT = false;
#include "bflbm_handover_body.inc"
}
// The quiet kernel for P.inv_tau_f_bar == P.inv_tau_g_bar == 1.0 (tau = 1/2): the same source with the relaxation's
// unit-rate form (d_relax_with<false, true>), under its own name so that k_fused_ho's symbols and code stay what they were.
template <int TY, bool RAG>
__global__ void __launch_bounds__(64 * TY, 1)
k_fused_ho_unit(const double* __restrict__ S, double* __restrict__ D, Geo G, DevParams P, FusedGrid F, HoGrid Hg, uint32_t noise_index) {
  constexpr int MODE = 0;
  constexpr bool UNIT = true;
#include "bflbm_handover_body.inc"
}

// lattices the hand-over kernel takes: at least one whole tile; a narrower last tile column / lower last tile row needs
// two lanes / rows (a ring site owned by a tile ONE site wide or high also collects from the tile beyond it, which the
// 3 x 3 lookup of the consumer does not reach, and its two edge roles must be different lanes / rows)
static inline bool handover_ok(const Geo& G) {
  return G.nx >= 64 && G.nx % 64 != 1 && G.ny >= HO_TY && G.ny % HO_TY != 1;
}
static inline bool handover_ragged(const Geo& G) { return G.nx % 64 != 0 || G.ny % HO_TY != 0; }
static inline size_t handover_frame_doubles(const Geo& G) {
  return (size_t)((G.nx + 63) / 64) * (size_t)((G.ny + HO_TY - 1) / HO_TY) * HoLayout<HO_TY>::REC * (size_t)G.nzs;
}

struct HoSig { int pa = -1, pb = -1, lz = -1, nchunks = -1, cstride = -1; long long step = -1;
  bool same_geometry(const HoSig& o) const { return pa == o.pa && pb == o.pb && lz == o.lz && nchunks == o.nchunks && cstride == o.cstride; } };

// fin/fout: frame buffers of the state read / written.  sig_in: what wrote fin (step == steps-1 required);
// sig_out: the signature of this launch's plan, which describes fout once the launch has succeeded.  returns the
// launch's error code
static inline hipError_t handover_launch(const double* S, double* D, const double* fin, double* fout, const Geo& G, const DevParams& P,
                                  int pa, int pb, long long steps, const HoSig& sig_in, HoSig& sig_out, int ncu, hipStream_t stream, int pair_len = 0, int mode = 0) {
  constexpr int TX = 64, TY = HO_TY;
  FusedGrid F;
  (void)launch_plan(3, G, pa, pb, pair_len, mode, ncu, F);
  HoSig sig;
  sig.pa = pa; sig.pb = pb; sig.lz = F.lz; sig.nchunks = F.nchunks; sig.cstride = F.cstride; sig.step = steps;
  HoGrid Hg;
  Hg.fin = fin; Hg.fout = fout;
  Hg.fplane = (long long)F.ncols * HoLayout<TY>::REC;
  Hg.use_frames = (sig_in.step == steps - 1 && sig_in.same_geometry(sig)) ? 1 : 0;
  dim3 grid((unsigned)(F.per_xcd * 8)), block(TX * TY);
  const uint32_t nidx = (uint32_t)steps;
  const bool rag = handover_ragged(G);
  if (mode == 1) { if (rag) hipLaunchKernelGGL((k_fused_ho<TY, 1, true>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx);
                   else     hipLaunchKernelGGL((k_fused_ho<TY, 1, false>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx); }
  else if (unit_rates(P)) {
                   if (rag) hipLaunchKernelGGL((k_fused_ho_unit<TY, true>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx);
                   else     hipLaunchKernelGGL((k_fused_ho_unit<TY, false>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx); }
  else           { if (rag) hipLaunchKernelGGL((k_fused_ho<TY, 0, true>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx);
                   else     hipLaunchKernelGGL((k_fused_ho<TY, 0, false>), grid, block, 0, stream, S, D, G, P, F, Hg, nidx); }
  sig_out = sig;
  return hipGetLastError();
}

#endif  // BFLBM_HANDOVER_H_
