// bflbm_spectrum.h -- spectrum traces: the structure factor of chosen pairs of hydrodynamic variables of every sample,
// binned into spherical shells in |q| or into |k| along one axis, recorded on the device as a time series for a lone
// single-slab context or every replica of a batch (include/bflbm.h, "Spectrum traces": the definition is stated there
// and only there).  The accumulators (bflbm_sf.h, bflbm_batch_sf.h) keep one running mean of the full 3-D spectrum; the
// observable of a coarsening mixture is S(k, t) per shell and its first moment, which until now was a field download
// and a numpy fftn per sample.
// A sample is, on the owner's stream and without a host synchronisation,
//   the dense transform of bflbm_spectra.h   the spectra hat[B][nspec][nk],
//   k_spectrum_bin                  stage 1: per chunk of the sorted list, pair and replica the weighted sum of
//                                   Re(a^ conj(b^)) / N, threads striding the chunk in index order, the tree of block_reduce,
//   k_spectrum_finish               stage 2: per bin, pair and replica the chunk sums in chunk order, into the slot.
// The list holds the half-spectrum indices sorted by (bin, index), 4 B each; a chunk never crosses a bin, so a record
// depends on the spectra and the chunk table alone.  No atomics, no LDS beyond the tree, no scratch.
// A ring of z-slabs takes its samples by the slab transform with one sorted list per slab (spectrum_tables::build_slab
// here, the rest in bflbm_spectrum_ring.h); the handle, the per-handle calls and the two binning kernels are the ones below.
// The lifecycle and the sample store are those of bflbm_recorder.h, selection and transforms those of bflbm_spectra.h.
// Included by bflbm.hip after bflbm_spectra.h (needs bflbm_ctx, bflbm_batch, block_reduce).
#ifndef BFLBM_SPECTRUM_H_
#define BFLBM_SPECTRUM_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

// ---- the tables: host code that needs nothing of the library (a stand-alone program may include this part alone) ---------
namespace spectrum_tables {

constexpr int kChunkLen = 2048;      // entries per chunk at most: 8 per thread of stage 1.  An untimed heuristic.

struct Chunk { long long begin; int len; int bin; };   // entries [begin, begin + len) of the sorted list, all of `bin`

struct Tables {
  int nbins = 0;
  std::vector<uint32_t> list;            // half-spectrum indices (mz * ny + my) * (nx/2+1) + mx sorted by (bin, index)
  std::vector<Chunk> chunks;             // in list order
  std::vector<int> bin_first;            // [nbins + 1]: the chunks of bin s are bin_first[s] ... bin_first[s+1]-1
  std::vector<long long> count;          // [nbins]: full-spectrum modes of the bin
  std::vector<double> q;                 // [nbins]
  int max_chunks_per_bin = 0;
};

inline uint64_t isqrt_u64(uint64_t v) {                  // floor(sqrt(v)), integers only
  uint64_t r = 0;
  for (uint64_t bit = 1ULL << 31; bit; bit >>= 1) { const uint64_t t = r | bit; if (t * t <= v) r = t; }
  return r;
}
inline uint64_t gcd_u64(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }

// L = lcm(nx, ny, nz) with 12 (L/2)^2 < 2^63, or 0 where that does not hold
inline uint64_t shell_lcm(int nx, int ny, int nz) {
  unsigned __int128 L = (unsigned)nx;
  for (int n : {ny, nz}) { L = L / gcd_u64((uint64_t)L, (uint64_t)n) * (unsigned)n; if (L >> 40) return 0; }
  const unsigned __int128 half = L / 2;
  if (12 * half * half >> 63) return 0;
  return (uint64_t)L;
}

// the shell of K2: the integer s >= 0 with (2s-1)^2 W^2 <= 4 K2 < (2s+1)^2 W^2
inline int shell_of(uint64_t K2, uint64_t W) {
  const unsigned __int128 four = (unsigned __int128)4 * K2, W2 = (unsigned __int128)W * W;
  uint64_t s = (isqrt_u64((uint64_t)four) / W + 1) / 2;
  while (s > 0 && (unsigned __int128)(2 * s - 1) * (2 * s - 1) * W2 > four) --s;
  while ((unsigned __int128)(2 * s + 1) * (2 * s + 1) * W2 <= four) ++s;
  return (int)s;
}

// kind 0 shells (L from shell_lcm, not 0), 1 / 2 / 3 |kx| / |ky| / |kz|; nk = (nx/2+1) ny nz <= 2^32.
// The slab form: the rows ky in [ky0, ky1) of the half spectrum only, as the slab of a ring holds them after its z
// transform.  The list then holds LOCAL indices (mz * nky + (my - ky0)) * (nx/2+1) + mx, nky = ky1 - ky0, sorted by
// (bin, local index); the bins are those of the whole box (nbins too), count and q cover the slab's own rows, and k = 0
// is left out on the slab that holds ky = 0.  build() is the slab form over all rows.
inline void build_slab(int nx, int ny, int nz, int ky0, int ky1, int kind, int zero_avg, uint64_t L, int chunk_len, Tables& T) {
  const int nxc = nx / 2 + 1, nky = ky1 - ky0;
  const long long nk = (long long)nxc * nky * nz;
  const uint64_t W = kind == 0 ? L / (uint64_t)std::max(nx, std::max(ny, nz)) : 1;
  const uint64_t ux = kind == 0 ? L / nx : 0, uy = kind == 0 ? L / ny : 0, uz = kind == 0 ? L / nz : 0;
  // |k| per index and, for the shells, the terms of K2 per axis
  std::vector<uint64_t> tx(nxc), ty(ny), tz(nz);
  for (int m = 0; m < nxc; ++m) { const uint64_t k = (uint64_t)m; tx[m] = kind == 0 ? (k * ux) * (k * ux) : k; }
  for (int m = 0; m < ny; ++m) { const uint64_t k = (uint64_t)std::min(m, ny - m); ty[m] = kind == 0 ? (k * uy) * (k * uy) : k; }
  for (int m = 0; m < nz; ++m) { const uint64_t k = (uint64_t)std::min(m, nz - m); tz[m] = kind == 0 ? (k * uz) * (k * uz) : k; }
  std::vector<int> bin((size_t)nk);
  for (int mz = 0; mz < nz; ++mz)
    for (int my = ky0; my < ky1; ++my) {
      int* row = bin.data() + ((size_t)mz * nky + (my - ky0)) * nxc;
      for (int mx = 0; mx < nxc; ++mx)
        row[mx] = kind == 0 ? shell_of(tx[mx] + ty[my] + tz[mz], W) : (int)(kind == 1 ? tx[mx] : (kind == 2 ? ty[my] : tz[mz]));
    }
  // the top bin of the whole box: every term is largest at its Nyquist index, and the bin does not decrease with a term
  const uint64_t mtx = tx[nxc - 1], mty = ty[ny / 2], mtz = tz[nz / 2];
  const int top = kind == 0 ? shell_of(mtx + mty + mtz, W) : (int)(kind == 1 ? mtx : (kind == 2 ? mty : mtz));
  T.nbins = top + 1;
  if (zero_avg && ky0 == 0) bin[0] = -1;                   // k = 0: neither summed nor counted
  // a counting sort keeps the index order inside a bin
  std::vector<long long> first((size_t)T.nbins + 1, 0);
  for (long long i = 0; i < nk; ++i) if (bin[(size_t)i] >= 0) first[(size_t)bin[(size_t)i] + 1] += 1;
  for (int s = 0; s < T.nbins; ++s) first[(size_t)s + 1] += first[(size_t)s];
  T.list.assign((size_t)first[(size_t)T.nbins], 0);
  T.count.assign((size_t)T.nbins, 0);
  T.q.assign((size_t)T.nbins, 0.);
  std::vector<long double> qsum((size_t)T.nbins, 0.L);
  {
    std::vector<long long> at(first.begin(), first.end() - 1);
    for (int mz = 0; mz < nz; ++mz)
      for (int my = ky0; my < ky1; ++my)
        for (int mx = 0; mx < nxc; ++mx) {
          const long long i = ((long long)mz * nky + (my - ky0)) * nxc + mx;
          const int s = bin[(size_t)i];
          if (s < 0) continue;
          T.list[(size_t)at[(size_t)s]++] = (uint32_t)i;
          const int w = (mx == 0 || 2 * mx == nx) ? 1 : 2;
          T.count[(size_t)s] += w;
          if (kind == 0) {
            const double fx = (double)mx / (double)nx, fy = (double)std::min(my, ny - my) / (double)ny, fz = (double)std::min(mz, nz - mz) / (double)nz;
            qsum[(size_t)s] += (long double)w * (long double)(2.0 * M_PI * std::sqrt(fx * fx + fy * fy + fz * fz));
          }
        }
  }
  const int naxis = kind == 1 ? nx : (kind == 2 ? ny : nz);
  for (int s = 0; s < T.nbins; ++s) {
    if (kind == 0) T.q[(size_t)s] = T.count[(size_t)s] ? (double)(qsum[(size_t)s] / (long double)T.count[(size_t)s]) : std::nan("");
    else T.q[(size_t)s] = 2.0 * M_PI * (double)s / (double)naxis;
  }
  // chunks of at most chunk_len entries that never cross a bin
  T.bin_first.assign((size_t)T.nbins + 1, 0);
  T.max_chunks_per_bin = 0;
  for (int s = 0; s < T.nbins; ++s) {
    T.bin_first[(size_t)s] = (int)T.chunks.size();
    for (long long b = first[(size_t)s]; b < first[(size_t)s + 1]; b += chunk_len)
      T.chunks.push_back(Chunk{b, (int)std::min<long long>(chunk_len, first[(size_t)s + 1] - b), s});
    T.max_chunks_per_bin = std::max(T.max_chunks_per_bin, (int)T.chunks.size() - T.bin_first[(size_t)s]);
  }
  T.bin_first[(size_t)T.nbins] = (int)T.chunks.size();
}

inline void build(int nx, int ny, int nz, int kind, int zero_avg, uint64_t L, int chunk_len, Tables& T) {
  build_slab(nx, ny, nz, 0, ny, kind, zero_avg, L, chunk_len, T);
}

}  // namespace spectrum_tables

#ifndef BFLBM_SPECTRUM_TABLES_ONLY

// the tables of one sorted list on a device, and the chunk sums of a ring's slab
struct SpectrumTables {
  int device = 0;
  long long nchunks = 0;
  uint32_t* d_list = nullptr;       // the sorted half-spectrum indices
  spectrum_tables::Chunk* d_chunks = nullptr;
  int* d_bin_first = nullptr;       // [nbins + 1]
  double* partial = nullptr;        // a ring's slab: [pair][chunk]; the bin sums [pair][bin] are its block of the gather
};

struct bflbm_spectrum : bflbm_sample_store {  // d_rec [capacity][nrep][npairs][nbins], d_stage [nrep][npairs][nchunks]
  int nx = 0, ny = 0, nz = 0;
  long long nsites = 0;
  int kind = 0, zero_avg = 0;
  SpectraSelection sel;             // source 0 hydrovs, 1 hydrovsbar
  int nbins = 0, max_chunks_per_bin = 0;
  long long nchunks = 0;
  std::vector<long long> count;     // [nbins]
  std::vector<double> q;            // [nbins]
  DenseSpectra T;                   // a lone context or a batch
  // a ring: one table per slab (slab d owns the rows of slabs.slab[d]), d_stage is [nslabs][npairs][nbins] on slab 0's
  // device, nchunks the slabs' total, max_chunks_per_bin the most of any (slab, bin); T stays empty
  std::vector<SpectrumTables> tab;  // [1] of a lone context or a batch
  SlabSpectra slabs;
  RingGather gather;                // slab d's bin sums [npairs][nbins] into block d of d_stage (slab 0 writes block 0 itself)
  bflbm_spectrum() : bflbm_sample_store("spectrum trace", "bflbm_spectrum") {}
  ~bflbm_spectrum() override {
    for (SpectrumTables& t : tab) {
      hipSetDevice(t.device);
      for (void* p : {(void*)t.d_list, (void*)t.d_chunks, (void*)t.d_bin_first, (void*)t.partial}) if (p) hipFree(p);
    }
  }
  int record() override;
  int record_ring();                // bflbm_spectrum_ring.h
};

namespace {

// the tables T on `device`, with npairs rows of chunk sums where a slab keeps its own (partial_pairs > 0)
int spectrum_tables_upload(SpectrumTables& t, const char* call, int device, const spectrum_tables::Tables& T, int partial_pairs) {
  t.device = device;
  t.nchunks = (long long)T.chunks.size();
  HIP_TRY(hipSetDevice(device));
  const size_t lb_ = std::max<size_t>(T.list.size(), 1) * sizeof(uint32_t);
  const size_t cb = std::max<size_t>(T.chunks.size(), 1) * sizeof(spectrum_tables::Chunk), bb = T.bin_first.size() * sizeof(int);
  const size_t pb = (size_t)partial_pairs * std::max<size_t>(T.chunks.size(), 1) * sizeof(double);
  hipError_t e = hipMalloc((void**)&t.d_list, lb_);
  if (e == hipSuccess) e = hipMalloc((void**)&t.d_chunks, cb);
  if (e == hipSuccess) e = hipMalloc((void**)&t.d_bin_first, bb);
  if (e == hipSuccess && pb) e = hipMalloc((void**)&t.partial, pb);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: out of device memory on device %d (index list %zu + chunk table %zu + bin table %zu + chunk sums %zu bytes): %s",
                call, device, lb_, cb, bb, pb, hipGetErrorString(e));
  }
  if (!T.list.empty()) HIP_TRY(hipMemcpy(t.d_list, T.list.data(), T.list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (!T.chunks.empty()) HIP_TRY(hipMemcpy(t.d_chunks, T.chunks.data(), T.chunks.size() * sizeof(spectrum_tables::Chunk), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(t.d_bin_first, T.bin_first.data(), bb, hipMemcpyHostToDevice));
  return 0;
}

// Stage 1, grid (chunks, pairs, B): the thread adds weight * (scale a^) . b^ / N of the chunk's entries tid, tid + 256, ...
// in that order (the product as k_sf_accumulate writes it; the weight, 1 or 2, is exact), the workgroup adds the 256
// partial sums by the tree of block_reduce into partial[replica][pair][chunk].
__global__ void __launch_bounds__(256) k_spectrum_bin(const double2* __restrict__ hat, const uint32_t* __restrict__ list,
                                                      const spectrum_tables::Chunk* __restrict__ chunks, double* __restrict__ partial,
                                                      long long nk, int nspec, int nx, SfPairs P, double inv_n) {
  const spectrum_tables::Chunk C = chunks[blockIdx.x];
  const int p = blockIdx.y;
  const double2* __restrict__ mine = hat + (long long)blockIdx.z * nspec * nk;
  const double2* __restrict__ A = mine + (long long)P.a[p] * nk;
  const double2* __restrict__ B = mine + (long long)P.b[p] * nk;
  const double s = P.scale[p];
  const uint32_t nxc = (uint32_t)(nx / 2 + 1);
  double v[1] = { 0. };
  for (int i = threadIdx.x; i < C.len; i += 256) {
    const uint32_t k = list[C.begin + i];
    const double2 a = A[k], b = B[k];
    const double ar = s * a.x, ai = s * a.y;
    const double t = (ar * b.x + ai * b.y) * inv_n;
    const uint32_t mx = k % nxc;
    v[0] += (mx == 0 || 2 * (int)mx == nx) ? t : 2. * t;      // -k lies in the same bin and adds the same real part
  }
  block_reduce<1>(v, partial + (long long)blockIdx.z * gridDim.y * gridDim.x);
}

// Stage 2, grid (ceil(nbins / 256), pairs, B): one thread per (bin, pair, replica) adds the bin's chunk sums in chunk
// order and writes the sample's [replica][pair][bin].  out = the slot of replica 0.
__global__ void __launch_bounds__(256) k_spectrum_finish(const double* __restrict__ partial, const int* __restrict__ bin_first,
                                                         double* __restrict__ out, int nbins, long long nchunks) {
  const int bin = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (bin >= nbins) return;
  const long long row = (long long)blockIdx.z * gridDim.y + blockIdx.y;          // replica * npairs + pair
  const double* __restrict__ mine = partial + row * nchunks;
  double acc = 0.;
  for (int c = bin_first[bin]; c < bin_first[bin + 1]; ++c) acc += mine[c];
  out[row * nbins + bin] = acc;
}

// what every creation call refuses about its own arguments ...
int spectrum_refuse_args(const char* call, int npairs, const int* var_a, const int* var_b, int lb_hydrovars, int kind,
                         int every, long long capacity) {
  if (npairs < 1 || npairs > 32) return fail("%s: 1..32 pairs (got %d)", call, npairs);
  if (field_refuse_pair_vars(call, lb_hydrovars ? 1 : 0, npairs, var_a, var_b)) return 1;
  if (kind < 0 || kind > 3) return fail("%s: kind must be 0 (shells), 1, 2 or 3 (axis x, y, z) (got %d)", call, kind);
  return store_refuse_cadence(call, every, capacity);
}
// ... and about the owner's box; *L: the lcm of the shells (1 for an axis)
int spectrum_refuse_box(const char* call, int kind, const Geo& G, uint64_t* L) {
  const int nx = G.nx, ny = G.ny, nz = G.nz;
  const long long nk = (long long)(nx / 2 + 1) * ny * nz;
  if (nk > (1LL << 32)) return fail("%s: the half spectrum of %d x %d x %d has %lld points, more than the 2^32 the index list holds", call, nx, ny, nz, nk);
  *L = kind == 0 ? spectrum_tables::shell_lcm(nx, ny, nz) : 1;
  if (!*L) return fail("%s: lcm(%d, %d, %d) is too large for shells: 12 (L/2)^2 must fit in 63 bits", call, nx, ny, nz);
  return 0;
}

// the box, the kind, where a pair's spectra lie and the bins of the whole box
void spectrum_select(bflbm_spectrum* t, const Geo& G, int npairs, const int* var_a, const int* var_b, const double* scale,
                     int lb_hydrovars, int kind, int zero_avg, const spectrum_tables::Tables& T) {
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz; t->nsites = (long long)G.nx * G.ny * G.nz;
  t->kind = kind; t->zero_avg = zero_avg ? 1 : 0;
  t->sel = spectra_select(lb_hydrovars ? 1 : 0, npairs, var_a, var_b, scale);
  t->nbins = T.nbins; t->count = T.count; t->q = T.q;
}

int spectrum_create(bflbm_ctx* c, bflbm_batch* b, int npairs, const int* var_a, const int* var_b, const double* scale,
                    int lb_hydrovars, int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out) {
  const char* call = b ? "bflbm_batch_spectrum_create" : "bflbm_spectrum_create";
  const Geo& G = c ? c->G : b->G;
  uint64_t L = 0;
  if (spectrum_refuse_args(call, npairs, var_a, var_b, lb_hydrovars, kind, every, capacity)) return 1;
  if (store_refuse_owner(c, call, "bflbm_batch_spectrum_create", "spectrum trace")) return 1;
  if (recorder_refuse_open(c, b, nullptr, call)) return 1;
  if (spectrum_refuse_box(call, kind, G, &L)) return 1;
  if (load_fft()) return 1;

  std::unique_ptr<bflbm_spectrum> t(new bflbm_spectrum());
  const int nrep = c ? 1 : (int)b->ctx.size();
  spectrum_tables::Tables T;
  spectrum_tables::build(G.nx, G.ny, G.nz, kind, zero_avg, L, spectrum_tables::kChunkLen, T);
  spectrum_select(t.get(), G, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, T);
  t->nchunks = (long long)T.chunks.size(); t->max_chunks_per_bin = T.max_chunks_per_bin;
  if (dense_create(t->T, call, c, b, t->sel.nspec)) return 1;
  t->tab.resize(1);
  if (spectrum_tables_upload(t->tab[0], call, t->T.device, T, 0)) return 1;
  const size_t per = (size_t)nrep * npairs * (size_t)T.nbins;
  const size_t stage = (size_t)nrep * npairs * std::max<size_t>(T.chunks.size(), 1);
  const std::string shape = " x " + std::to_string(npairs) + " pairs x " + std::to_string(T.nbins) + " bins";
  if (store_attach(t.get(), c, b, call, every, capacity, per, stage, shape.c_str())) return 1;
  *out = t.release();
  return 0;
}

}  // namespace

// enqueue the observation, the transforms and the two binning stages of the resident state into slot n; no host synchronisation
int bflbm_spectrum::record() {
  if (ring) return record_ring();
  if (store_begin(this)) return 1;
  const hipStream_t stream = recorder_stream(this);
  if (dense_run(T, this, sel.fs, sel.vars, "spectrum trace sample")) return 1;
  const SfPairs& pairs = sel.pairs;
  if (nchunks > 0) {
    hipLaunchKernelGGL(k_spectrum_bin, dim3((unsigned)nchunks, (unsigned)pairs.n, (unsigned)nrep), dim3(256), 0, stream,
                       T.hat, tab[0].d_list, tab[0].d_chunks, d_stage, T.nk, sel.nspec, nx, pairs, 1.0 / (double)nsites);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_spectrum_finish, dim3((unsigned)((nbins + 255) / 256), (unsigned)pairs.n, (unsigned)nrep), dim3(256), 0, stream,
                     d_stage, tab[0].d_bin_first, store_slot(this), nbins, std::max(nchunks, 1LL));
  HIP_TRY(hipGetLastError());
  store_recorded(this);
  return 0;
}

extern "C" {

int bflbm_spectrum_create(bflbm_ctx* c, int npairs, const int* var_a, const int* var_b, const double* scale, int lb_hydrovars,
                          int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out) {
  if (!c || !var_a || !var_b || !out) return fail("bflbm_spectrum_create: null argument");
  return spectrum_create(c, nullptr, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, every, capacity, out);
}
int bflbm_batch_spectrum_create(bflbm_batch* b, int npairs, const int* var_a, const int* var_b, const double* scale, int lb_hydrovars,
                                int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out) {
  if (!b || !var_a || !var_b || !out) return fail("bflbm_batch_spectrum_create: null argument");
  return spectrum_create(nullptr, b, npairs, var_a, var_b, scale, lb_hydrovars, kind, zero_avg, every, capacity, out);
}

int bflbm_spectrum_destroy(bflbm_spectrum* t) { return store_destroy(t); }
int bflbm_spectrum_sample(bflbm_spectrum* t) { return store_sample(t, "bflbm_spectrum"); }
int bflbm_spectrum_reset(bflbm_spectrum* t) { return store_reset(t, "bflbm_spectrum"); }
int bflbm_spectrum_count(const bflbm_spectrum* t, long long* nsamples, int* nreplicas) { return store_count(t, "bflbm_spectrum", nsamples, nreplicas); }
int bflbm_spectrum_read(bflbm_spectrum* t, long long first, long long count, double* sums, long long* steps) {
  return store_read(t, "bflbm_spectrum", first, count, sums, steps);
}

int bflbm_spectrum_geometry(const bflbm_spectrum* t, int* nbins, int* npairs, long long* nchunks, int* max_chunks_per_bin) {
  if (!t) return fail("bflbm_spectrum_geometry: null argument");
  if (nbins) *nbins = t->nbins;
  if (npairs) *npairs = t->sel.pairs.n;
  if (nchunks) *nchunks = t->nchunks;
  if (max_chunks_per_bin) *max_chunks_per_bin = t->max_chunks_per_bin;
  return 0;
}

int bflbm_spectrum_bins(const bflbm_spectrum* t, long long* count, double* q) {
  if (!t) return fail("bflbm_spectrum_bins: null argument");
  if (count) std::copy(t->count.begin(), t->count.end(), count);
  if (q) std::copy(t->q.begin(), t->q.end(), q);
  return 0;
}

}  // extern "C"

#endif  // BFLBM_SPECTRUM_TABLES_ONLY

#endif  // BFLBM_SPECTRUM_H_
