// bflbm_chord.h -- chord traces: the run-length distributions along x, y and z of the set {v >= level} or {v < level} of
// one observed hydrovs or hydrovsbar variable at 1 to 8 levels, recorded on the device as a time series of 64-bit integer
// counts for a lone single-slab context or every replica of a batch (include/bflbm.h, "Chord traces": the rule and the
// layout of a sample are stated there and only there).  The mean chord per axis is the stereological domain size, the
// tail tells a sponge from droplets and the three axes against each other show anisotropy, which the shell spectrum and
// the Minkowski counts average away; without this a user downloads the field per sample and walks its lines on the host.
// A sample is, on the owner's stream and without a host synchronisation,
//   the accumulators' observation   of the one variable, exactly as the morphology trace takes it (fields_observe),
//   k_chord_rows<NL>                the x launch, grid (groups, 1, replicas), 256 threads: a wave takes a row of nx
//                                   contiguous sites 64 at a turn (the next block's load is issued before this block's
//                                   bits are worked on).  Per level one __ballot gives the block's occupancy mask m and
//                                   z = ~m within the row its unoccupied sites.  A run closes at a zero whose predecessor
//                                   is occupied: the lanes of z & (m << 1), plus lane 0 where the run carried in from
//                                   the blocks before ends there.  Such a lane finds its run's length by bit
//                                   operations: the distance to the highest zero below it, or, for the block's first
//                                   zero, the carried length plus its own lane.  The open run (the ones after the
//                                   block's last zero, or the whole block on top of what was open) is carried to the
//                                   next block as a wave-uniform length.  The run that ends at the row's first zero is
//                                   the run through site 0: it is kept apart and joined with the run that is still open
//                                   at nx - 1 when the row is finished.  A row without a zero is a spanning line.  The
//                                   occupied sites V are counted here too, one population count per block and level,
//   k_chord_march<NL>               the y and the z launch, one kernel, the stride along the axis and the line map as
//                                   arguments: grid (groups, 1, replicas), 256 threads, a work item is 256 consecutive
//                                   lines p = o nx + x (o = z for the y launch, o = y for the z launch), so the lanes lie
//                                   along x and every load is a coalesced row segment.  A lane marches its line from 0
//                                   to n_a - 1, eight loads in flight, and keeps per level the open run, the head run
//                                   (the run before its first zero) and a bit "a zero was seen" in registers; head and
//                                   tail are joined at the end, a line without a zero is a spanning line,
//   k_hist_finish                   the histogram trace's finishing launch, shared: the totals into the slot
//                                   [sample][replica][nlevels][W], and the totals back to zero for the next sample.
// Counters: a closed chord adds 1 to its bin, and its length to long_sites where it lands in the last bin, with LDS
// atomics into a workgroup's private copy of the record, [nlevels][W] 32-bit words of dynamic LDS (4 nlevels W bytes, at
// most 64 KiB: two workgroups of the largest record fit a CU's 160 KiB).  `chords`, `spanning` and V are
// population counts of wave ballots added into wave-uniform 32-bit registers and reach LDS once per wave at the end.  Then
// one 64-bit global add per non-zero counter and workgroup, as k_hist_count does.  Integer sums commute, so the record is
// exact whatever the launch geometry.  No scratch, no grid barrier, no atomics other than the LDS adds and the flush.
// A line is handled whole by one wave (x) or one lane (y, z); lines are not cut into chunks, there is no merge pass.
// The 32-bit counters: no counter of a workgroup can pass the sites the workgroup meets (a chord adds 1 to a bin and its
// length, at most the sites it covers, to long_sites).  The host chooses the groups so that a workgroup meets at most
// 2^30 sites or one work item (four rows, or 256 lines), whichever is more; a work item holds at most
// min(nsites, 256 x extent) sites, so a counter could wrap only in a box of 2^31 sites with an extent of 2^23, which no
// device holds.  The run lengths themselves are below an extent, an int.
// The level count is a template parameter, NL = 1 .. 8, compiled once each: the per-level state (open, head, the
// wave-uniform counts) is indexed statically and stays in registers.  All levels share a loaded value.  The side is a
// runtime value (morph_mask's exclusive-or).
// Expected memory traffic, derived: the observed field is read once per axis, 3 x 8 = 24 bytes per site and sample,
// against the 608 of a step; the x launch reads whole rows, the marches whole row segments of at least min(nx, 64)
// sites.  What the compiler reports (gfx950, -O3), NL = 1 / 3 / 8: k_chord_rows 22 / 26 / 41 VGPRs and
// 59 / 89 / 106 SGPRs, k_chord_march 34 / 38 / 88 VGPRs and 85 / 106 / 106 SGPRs (occupancy 8 / 7 / 5 waves per SIMD);
// LDSByteSize 0 (no static LDS: the counters are the launch's dynamic LDS) and ScratchSize 0 in all sixteen
// (tests/test_chord_abi.py reads both from the listing).
// Groups: min(work items, 2048 / replicas) and the bound above; a workgroup strides over the work items.  The 2048 (eight
// workgroups per CU of 256) and the eight loads in flight are untimed heuristics.
// No ring: a z chord crosses the slab boundaries, possibly all of them, and a slab holds its own planes only; there is no
// bflbm_ring_chord_create.  Not built on purpose: chords along diagonals, chords of a second variable, both sides in one
// trace, fusing the count into the observation.
// Host part: plain C++17 on top of bflbm_morph.h's host part (the levels, their refusals, the plane limit) and
// bflbm_hist.h's counter cap.  A stand-alone program defines BFLBM_CHORD_HOST_ONLY (and the MORPH, HIST and FIELDSEL ones)
// and includes it after bflbm_hist.h and bflbm_morph.h (tests/chord_main.cpp).  HIP part: the lifecycle and the sample
// store are those of bflbm_recorder.h, the selection that of bflbm_fieldsel.h.  Included by bflbm.hip after bflbm_morph.h
// (needs bflbm_ctx, bflbm_batch, FieldSelection, fields_observe, field_dispatch_nv, morph_mask, k_hist_finish).
#ifndef BFLBM_CHORD_H_
#define BFLBM_CHORD_H_

#include <algorithm>

namespace chord_limits {
constexpr int kMaxLength = 4096;                         // M, the last bin
constexpr int kMaxCounters = hist_limits::kMaxCounters;  // nlevels x W 32-bit counters: 64 KiB of LDS, the histogram trace's cap
constexpr int kRowsPerItem = 4;                          // the x launch: a row per wave
constexpr int kLinesPerItem = 256;                       // the y and z launches: a line per lane
constexpr int kGroups = 2048;                            // workgroups of a launch over all replicas (eight per CU of 256)
constexpr long long kMaxGroupSites = 1LL << 30;          // the sites a workgroup meets, or one work item where that is more
constexpr int kInFlight = 8;                             // loads of a marching lane in flight
}

// the layout of a level's W words and the launch shapes; a by-value kernel parameter
struct ChordLayout {
  int M, W;                          // max_length; W = 1 + 3 (3 + M)
};

namespace {

// words of a level: V, then per axis chords, spanning, long_sites, h[1..M]
constexpr int chord_words(int max_length) { return 1 + 3 * (3 + max_length); }
// offset of axis a's block within a level's words (constexpr: the kernels call it too)
constexpr int chord_block(int max_length, int axis) { return 1 + axis * (3 + max_length); }

// What every creation call refuses about its arguments, in the order of include/bflbm.h: the morphology trace's refusals,
// then max_length, then the counters of a workgroup.
int chord_refuse_args(const char* call, int source, int var, int nlevels, const double* levels, int side, int max_length) {
  using namespace chord_limits;
  if (morph_refuse_args(call, source, var, nlevels, levels, side)) return 1;
  if (max_length < 1 || max_length > kMaxLength) return fail("%s: max_length in 1..%d (got %d)", call, kMaxLength, max_length);
  const long long counters = (long long)nlevels * chord_words(max_length);
  if (counters > kMaxCounters)
    return fail("%s: %d levels x %d words = %lld counters per replica exceed %d", call, nlevels, chord_words(max_length), counters, kMaxCounters);
  return 0;
}

// work items of a launch along `axis` (0 x: four rows each, 1 y and 2 z: 256 lines each) and the sites of one
inline long long chord_items(int axis, int nx, int ny, int nz) {
  using namespace chord_limits;
  if (axis == 0) return ((long long)ny * nz + kRowsPerItem - 1) / kRowsPerItem;
  return ((long long)nx * (axis == 1 ? nz : ny) + kLinesPerItem - 1) / kLinesPerItem;
}
inline long long chord_item_sites(int axis, int nx, int ny, int nz) {
  using namespace chord_limits;
  if (axis == 0) return std::min<long long>(kRowsPerItem, (long long)ny * nz) * nx;
  return std::min<long long>(kLinesPerItem, (long long)nx * (axis == 1 ? nz : ny)) * (axis == 1 ? ny : nz);
}
// workgroups per replica of the launch along `axis`: no workgroup meets more than kMaxGroupSites sites, or one work item
inline long long chord_groups(int axis, int nx, int ny, int nz, int nrep) {
  using namespace chord_limits;
  const long long items = chord_items(axis, nx, ny, nz);
  const long long per_group = std::max<long long>(1, kMaxGroupSites / chord_item_sites(axis, nx, ny, nz));
  const long long want = std::min<long long>(items, std::max(1, kGroups / nrep));
  return std::max(want, (items + per_group - 1) / per_group);
}

}  // namespace

#ifndef BFLBM_CHORD_HOST_ONLY

#include <memory>
#include <string>

struct bflbm_chord : bflbm_sample_store {    // d_rec [capacity][nrep][nlevels][W] as long long, d_stage: the totals [nrep][nlevels][W]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar; one variable
  MorphLevels L;
  ChordLayout Y;
  double* fields = nullptr;         // a batch: [nrep][nsites]
  bflbm_chord() : bflbm_sample_store("chord trace", "bflbm_chord") {}
  ~bflbm_chord() override {
    if (fields) { hipSetDevice(device); hipFree(fields); }
  }
  unsigned long long* totals() const { return reinterpret_cast<unsigned long long*>(d_stage); }
  int record() override;
};

namespace {

// a closed chord of `len` >= 1 sites into the axis block `blk` (chords, spanning, long_sites, h[1..M]) of a level in LDS
__device__ __forceinline__ void chord_add(unsigned* __restrict__ blk, int len, int M) {
  atomicAdd(&blk[2 + min(len, M)], 1u);
  if (len >= M) atomicAdd(&blk[2], (unsigned)len);
}

// the workgroup's counters into the replica's totals: one 64-bit add per non-zero counter
__device__ __forceinline__ void chord_flush(const unsigned* __restrict__ sh, int C, unsigned long long* __restrict__ totals) {
  unsigned long long* __restrict__ mine = totals + (long long)blockIdx.z * C;
  for (int i = (int)threadIdx.x; i < C; i += 256) {
    const unsigned n = sh[i];
    if (n) atomicAdd(&mine[i], (unsigned long long)n);
  }
}

// grid (groups, 1, replicas), 256 threads, 4 NL W bytes of dynamic LDS.  field: the dense volume [rows][nx] of replica r
// at field + r rep_stride, rows = ny nz; totals: [replica][NL][W].  Fills word 0 and the x block of every level.
template <int NL>
__global__ void __launch_bounds__(256) k_chord_rows(const double* __restrict__ field, long long rep_stride, int nx, long long rows,
                                                    unsigned long long* __restrict__ totals, MorphLevels L, ChordLayout Y) {
  extern __shared__ unsigned chord_sh[];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = NL * Y.W;
  for (int i = tid; i < C; i += 256) chord_sh[i] = 0u;
  __syncthreads();
  const double* __restrict__ vol = field + (long long)blockIdx.z * rep_stride;
  const unsigned flip = L.side ? (1u << NL) - 1u : 0u;
  const unsigned long long below = (1ull << lane) - 1ull;          // the lanes below this one
  const int xblk = chord_block(Y.M, 0);
  unsigned nocc[NL], nch[NL], nspan[NL];                            // wave-uniform
#pragma unroll
  for (int l = 0; l < NL; ++l) { nocc[l] = 0u; nch[l] = 0u; nspan[l] = 0u; }

  for (long long row = (long long)blockIdx.x * chord_limits::kRowsPerItem + wave; row < rows; row += (long long)gridDim.x * chord_limits::kRowsPerItem) {
    const double* __restrict__ r = vol + row * nx;
    int open[NL], head[NL];                                         // wave-uniform: the run open at the block's end; the run before the first zero
    unsigned any = 0u;                                              // bit l: a zero was seen at level l
#pragma unroll
    for (int l = 0; l < NL; ++l) { open[l] = 0; head[l] = 0; }
    double v = lane < nx ? r[lane] : 0.;
    for (int x0 = 0; x0 < nx; x0 += 64) {
      const int nb = min(64, nx - x0);                              // the block's sites: lanes 0 .. nb - 1
      const unsigned mk = lane < nb ? morph_mask<NL>(v, L, flip) : 0u;
      if (x0 + 64 + lane < nx) v = r[x0 + 64 + lane];               // the next block, in flight while this one is counted
      const unsigned long long valid = nb == 64 ? ~0ull : (1ull << nb) - 1ull;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const unsigned long long m = __ballot((int)((mk >> l) & 1u));
        const unsigned long long z = ~m & valid;
        nocc[l] += (unsigned)__popcll(m);
        if (z == 0ull) {                                            // no zero: the whole block goes on top of the open run
          open[l] += nb;
        } else {
          const int f = __builtin_ctzll(z), p = 63 - __builtin_clzll(z);      // the block's first and last zero
          // the zeros that close a run: an occupied site below them, or, for lane 0, a run carried in
          unsigned long long closing = z & (m << 1);
          if (f == 0 && open[l] > 0) closing |= 1ull;
          if (!((any >> l) & 1u)) {                                 // the row's first zero: what ends here is the run through site 0
            closing &= ~(1ull << f);
            head[l] = open[l] + f;
            any |= 1u << l;
          }
          nch[l] += (unsigned)__popcll(closing);
          if ((closing >> lane) & 1ull) {
            const unsigned long long lowz = z & below;
            const int len = lowz ? lane - 64 + __builtin_clzll(lowz) : open[l] + lane;      // lane - 1 - (63 - clz): from the zero below
            chord_add(chord_sh + l * Y.W + xblk, len, Y.M);
          }
          open[l] = nb - 1 - p;
        }
      }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {                                  // the row is finished: the seam
      if (!((any >> l) & 1u)) {
        nspan[l] += 1u;
      } else {
        const int tail = open[l] + head[l];                         // the run that ends at nx - 1 and the run through site 0: one chord
        if (tail > 0) {
          nch[l] += 1u;
          if (lane == 0) chord_add(chord_sh + l * Y.W + xblk, tail, Y.M);
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (nocc[l]) atomicAdd(&chord_sh[l * Y.W], nocc[l]);
      if (nch[l]) atomicAdd(&chord_sh[l * Y.W + xblk], nch[l]);
      if (nspan[l]) atomicAdd(&chord_sh[l * Y.W + xblk + 1], nspan[l]);
    }
  }
  __syncthreads();
  chord_flush(chord_sh, C, totals);
}

// grid (groups, 1, replicas), 256 threads, 4 NL W bytes of dynamic LDS.  Line p = o nx + x of `nlines` starts at
// o ostride + x and has n sites `astride` apart (y: o = z, ostride = nx ny, astride = nx, n = ny; z: o = y, ostride = nx,
// astride = nx ny, n = nz).  Fills the block at `blk` of every level.
template <int NL>
__global__ void __launch_bounds__(256) k_chord_march(const double* __restrict__ field, long long rep_stride, int nx, long long nlines, int n,
                                                     long long astride, long long ostride, int blk,
                                                     unsigned long long* __restrict__ totals, MorphLevels L, ChordLayout Y) {
  using namespace chord_limits;
  extern __shared__ unsigned chord_sh[];
  const int tid = (int)threadIdx.x;
  const int C = NL * Y.W;
  for (int i = tid; i < C; i += 256) chord_sh[i] = 0u;
  __syncthreads();
  const double* __restrict__ vol = field + (long long)blockIdx.z * rep_stride;
  const unsigned flip = L.side ? (1u << NL) - 1u : 0u;
  unsigned nch[NL], nspan[NL];                                      // wave-uniform
#pragma unroll
  for (int l = 0; l < NL; ++l) { nch[l] = 0u; nspan[l] = 0u; }

  const long long items = (nlines + kLinesPerItem - 1) / kLinesPerItem;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long p = item * kLinesPerItem + tid;
    const bool in = p < nlines;                                     // a lane past the lines marches line 0 and occupies nothing
    const long long pc = in ? p : 0;
    const long long o = pc / nx;
    const double* __restrict__ line = vol + o * ostride + (pc - o * nx);
    int open[NL], head[NL];
    unsigned any = in ? 0u : (1u << NL) - 1u;                       // no line: a zero was seen, no run ever opens
#pragma unroll
    for (int l = 0; l < NL; ++l) { open[l] = 0; head[l] = 0; }
    auto site = [&](double v) {
      const unsigned mk = in ? morph_mask<NL>(v, L, flip) : 0u;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const bool occ = (mk >> l) & 1u, had = (any >> l) & 1u;
        const bool close = !occ && had && open[l] > 0;
        nch[l] += (unsigned)__popcll(__ballot((int)close));
        if (close) chord_add(chord_sh + l * Y.W + blk, open[l], Y.M);
        if (!occ && !had) { head[l] = open[l]; any |= 1u << l; }    // the line's first zero: what ends here is the run through site 0
        open[l] = occ ? open[l] + 1 : 0;
      }
    };
    int k = 0;
    for (; k + kInFlight <= n; k += kInFlight) {
      double v[kInFlight];
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) v[j] = line[(long long)(k + j) * astride];
#pragma unroll
      for (int j = 0; j < kInFlight; ++j) site(v[j]);
    }
    for (; k < n; ++k) site(line[(long long)k * astride]);
#pragma unroll
    for (int l = 0; l < NL; ++l) {                                  // the line is finished: the seam
      const bool had = (any >> l) & 1u;
      const int tail = open[l] + head[l];
      const bool close = had && tail > 0;
      nspan[l] += (unsigned)__popcll(__ballot((int)!had));
      nch[l] += (unsigned)__popcll(__ballot((int)close));
      if (close) chord_add(chord_sh + l * Y.W + blk, tail, Y.M);
    }
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      if (nch[l]) atomicAdd(&chord_sh[l * Y.W + blk], nch[l]);
      if (nspan[l]) atomicAdd(&chord_sh[l * Y.W + blk + 1], nspan[l]);
    }
  }
  __syncthreads();
  chord_flush(chord_sh, C, totals);
}

int chord_create(bflbm_ctx* c, bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int max_length, int every,
                 long long capacity, bflbm_chord** out) {
  const char* call = b ? "bflbm_batch_chord_create" : "bflbm_chord_create";
  if (chord_refuse_args(call, source, var, nlevels, levels, side, max_length)) return 1;
  const Geo& G = c ? c->G : b->G;
  if ((long long)G.nx * G.ny > morph_limits::kMaxPlane)
    return fail("%s: a plane of %lld sites exceeds %lld", call, (long long)G.nx * G.ny, morph_limits::kMaxPlane);
  if (store_refuse_owner(c, call, "bflbm_batch_chord_create", "chord trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  if (store_refuse_cadence(call, every, capacity)) return 1;

  std::unique_ptr<bflbm_chord> t(new bflbm_chord());
  recorder_bind(t.get(), c, b, every);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->fs = field_select(b != nullptr, source, 1, &var);
  t->L = morph_levels(nlevels, levels, side);
  t->Y.M = max_length; t->Y.W = chord_words(max_length);

  const size_t per = (size_t)t->nrep * nlevels * t->Y.W;
  const std::string shape = " x " + std::to_string(nlevels) + " levels x " + std::to_string(t->Y.W) + " words";
  if (store_refuse_capacity(call, capacity, per, t->nrep, shape.c_str())) return 1;      // before the field of a batch
  const size_t sb = per * sizeof(long long);
  const size_t fb = b ? (size_t)t->nrep * (size_t)t->nsites * sizeof(double) : 0;
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess && fb) e = hipMalloc((void**)&t->fields, fb);
  if (e != hipSuccess) {                                     // the destructors free what was allocated
    (void)hipGetLastError();
    return fail("%s: out of device memory (field %zu bytes; then records %zu x %lld + totals %zu): %s", call, fb, sb, capacity, sb, hipGetErrorString(e));
  }
  if (store_attach(t.get(), c, b, call, every, capacity, per, per, shape.c_str())) return 1;
  // the totals are the store's stage buffer: zeroed after the owner's list took the trace, as the morphology trace does
  bflbm_chord* m = t.release();
  e = hipMemsetAsync(m->d_stage, 0, sb, recorder_stream(m));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    store_destroy(m);
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  *out = m;
  return 0;
}

}  // namespace

// enqueue the observation, the three counting launches and the finishing launch of the resident state into slot n; no host
// synchronisation
int bflbm_chord::record() {
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  const double* dense;
  long long rep_stride;
  if (fields_observe(this, fs, fields, "chord trace sample", &dense, &rep_stride)) return 1;
  const double* vol = dense + (long long)fs.vol.vol[0] * nsites;
  const long long plane = (long long)nx * ny;
  const size_t lds = (size_t)L.n * Y.W * sizeof(unsigned);
  const dim3 gx((unsigned)chord_groups(0, nx, ny, nz, nrep), 1, (unsigned)nrep), gy((unsigned)chord_groups(1, nx, ny, nz, nrep), 1, (unsigned)nrep),
      gz((unsigned)chord_groups(2, nx, ny, nz, nrep), 1, (unsigned)nrep);
  if (!field_dispatch_nv(L.n, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        hipLaunchKernelGGL((k_chord_rows<NL>), gx, dim3(256), lds, stream, vol, rep_stride, nx, (long long)ny * nz, totals(), L, Y);
        hipLaunchKernelGGL((k_chord_march<NL>), gy, dim3(256), lds, stream, vol, rep_stride, nx, (long long)nx * nz, ny, (long long)nx, plane,
                           chord_block(Y.M, 1), totals(), L, Y);
        hipLaunchKernelGGL((k_chord_march<NL>), gz, dim3(256), lds, stream, vol, rep_stride, nx, plane, nz, plane, (long long)nx,
                           chord_block(Y.M, 2), totals(), L, Y);
      })) return fail("chord trace: %d levels", L.n);
  HIP_TRY(hipGetLastError());
  const int n = nrep * L.n * Y.W;
  hipLaunchKernelGGL(k_hist_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     totals(), reinterpret_cast<long long*>(store_slot(this)), n, (const long long*)nullptr, 0);
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_chord_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels, int side, int max_length, int every,
                       long long capacity, bflbm_chord** out) {
  if (!c || !levels || !out) return fail("bflbm_chord_create: null argument");
  return chord_create(c, nullptr, source, var, nlevels, levels, side, max_length, every, capacity, out);
}
int bflbm_batch_chord_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side, int max_length, int every,
                             long long capacity, bflbm_chord** out) {
  if (!b || !levels || !out) return fail("bflbm_batch_chord_create: null argument");
  return chord_create(nullptr, b, source, var, nlevels, levels, side, max_length, every, capacity, out);
}

int bflbm_chord_destroy(bflbm_chord* t) { return store_destroy(t); }
int bflbm_chord_sample(bflbm_chord* t) { return store_sample(t, "bflbm_chord"); }
int bflbm_chord_reset(bflbm_chord* t) { return store_reset(t, "bflbm_chord"); }
int bflbm_chord_count(const bflbm_chord* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_chord", nsamples, nreplicas); }
int bflbm_chord_read(bflbm_chord* t, long long first, long long count, long long* counts, long long* steps) {
  return store_read(t, "bflbm_chord", first, count, reinterpret_cast<double*>(counts), steps);   // 8-byte slots, copied bit for bit
}

int bflbm_chord_geometry(const bflbm_chord* t, int* nlevels, int* max_length, int* words, int* lds_counters, int* groups_x, int* groups_y,
                         int* groups_z) {
  if (!t) return fail("bflbm_chord_geometry: null argument");
  if (nlevels) *nlevels = t->L.n;
  if (max_length) *max_length = t->Y.M;
  if (words) *words = t->Y.W;
  if (lds_counters) *lds_counters = t->L.n * t->Y.W;
  if (groups_x) *groups_x = (int)(chord_groups(0, t->nx, t->ny, t->nz, t->nrep) * t->nrep);
  if (groups_y) *groups_y = (int)(chord_groups(1, t->nx, t->ny, t->nz, t->nrep) * t->nrep);
  if (groups_z) *groups_z = (int)(chord_groups(2, t->nx, t->ny, t->nz, t->nrep) * t->nrep);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_CHORD_HOST_ONLY

#endif  // BFLBM_CHORD_H_
