// bflbm_fstat.h -- field statistics: per-site running sums over frames of chosen hydrovs, hydrovsbar or noise components
// and of chosen products of their deviations from the first frame, for a lone single-slab context, every replica of a
// batch or a ring of z-slabs (include/bflbm.h, "Field statistics": the definition is stated there and only there).
// The mean of a field at every site and the second moments around it are what PrintConvergence and the reference's own
// noise check form (Debug.H:275-358, NoiseCovariance.ipynb cell 3); without this a user downloads full fields frame by
// frame.  A sample is, on the owner's stream(s) and without a host synchronisation,
//   the accumulators' observation   batch_observe_launch into the recorder's [B][nvars][n] / observe_launch into the
//                                   scratch state buffer of the context (of every slab of a ring),
//   k_fstat_accumulate<NV>          one launch over the dense sites: a thread takes two neighbouring sites per turn, loads
//                                   the chosen variables once, updates sum, writes first on frame 0, updates every prod.
// A per-site accumulator never crosses a slab boundary: on a ring every slab keeps the accumulators of its own planes on
// its own device and feeds them on its own stream, with no event between the slabs.  No atomics, no LDS, no scratch.
// Not built on purpose: the L1 deviation of PrintConvergence (two passes over stored frames), a noise source on batches
// (k_observe_batch has no noise form), windows that forget old frames, fusing the accumulation into the observation
// kernels (it would give every observer a second form).
// The lifecycle is that of bflbm_recorder.h, the selection that of bflbm_fieldsel.h; capacity is unbounded, every = 0 is
// fed by hand only.  Included by bflbm.hip after bflbm_modes.h (needs bflbm_ctx, bflbm_batch, bflbm_ring, FieldSelection,
// FstatVars, FstatPairs, fields_observe, field_dispatch_nv, ring_prepare_ref).
#ifndef BFLBM_FSTAT_H_
#define BFLBM_FSTAT_H_

#include <cstdint>
#include <memory>
#include <vector>

namespace fstat_limits {
constexpr int kMaxBlocks = 2048;     // the grid of the accumulation: at most this many workgroups, which stride the rest
}

// the accumulators of one owner part: the lone context, the batch, or one slab of a ring
struct FstatPart {
  int device = 0;
  int z0 = 0;                       // first global plane
  long long n = 0;                  // dense sites of the part: planes x ny x nx
  double* acc = nullptr;            // [nrep][2 nvars + npairs][n]: sum[v], first[v], prod[p]
  double* out = nullptr;            // [n]: what bflbm_fstat_get downloads
};

struct bflbm_fstat : bflbm_recorder {   // n: frames taken
  int nx = 0, ny = 0, nz = 0;
  FieldSelection fs;                // source 0 hydrovs, 1 hydrovsbar, 2 noise
  FstatPairs pairs;
  double* fields = nullptr;         // a batch: [nrep][nvars][n]
  std::vector<FstatPart> part;
  int nvol() const { return 2 * fs.nvars + pairs.n; }
  bflbm_fstat() : bflbm_recorder("field statistic", "bflbm_fstat") {}
  ~bflbm_fstat() override {
    for (FstatPart& q : part) {
      if (!q.acc && !q.out) continue;
      hipSetDevice(q.device);
      if (q.acc) hipFree(q.acc);
      if (q.out) hipFree(q.out);
    }
    if (fields) { hipSetDevice(device); hipFree(fields); }
  }
  int record() override;
};

namespace {

// W doubles from p: one 16-byte access where the volume is 16-byte aligned (the site index is even on this path)
template <int W> __device__ __forceinline__ void fstat_load(const double* __restrict__ p, bool aligned, double (&v)[W]) {
  if (W == 2 && aligned) { const double2 t = *reinterpret_cast<const double2*>(p); v[0] = t.x; v[W - 1] = t.y; }
  else {
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = p[i];
  }
}
template <int W> __device__ __forceinline__ void fstat_store(double* __restrict__ p, bool aligned, const double (&v)[W]) {
  if (W == 2 && aligned) *reinterpret_cast<double2*>(p) = make_double2(v[0], v[W - 1]);
  else {
#pragma unroll
    for (int i = 0; i < W; ++i) p[i] = v[i];
  }
}
__device__ __forceinline__ bool fstat_aligned(const double* p) { return ((uintptr_t)p & 15u) == 0; }

// entry k of a register array, k uniform over the workgroup: a chain of selects, never an indexed private array
template <int NV, int W> __device__ __forceinline__ void fstat_pick(const double (&d)[NV][W], int k, double (&r)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) r[i] = d[0][i];
#pragma unroll
  for (int v = 1; v < NV; ++v) {
#pragma unroll
    for (int i = 0; i < W; ++i) r[i] = (k == v) ? d[v][i] : r[i];
  }
}

// the W sites s .. s + W - 1 of one replica: src the observation's volumes, acc the replica's accumulators
template <int NV, int W>
__device__ __forceinline__ void fstat_sites(const double* __restrict__ src, double* __restrict__ acc, long long n, long long s,
                                            const FstatVars& V, const FstatPairs& P, bool first_frame) {
  double dev[NV][W];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double* __restrict__ xs = src + (long long)V.vol[v] * n;
    double* __restrict__ sum = acc + (long long)v * n;
    double* __restrict__ fst = acc + (long long)(NV + v) * n;
    double x[W], f[W], t[W];
    fstat_load<W>(xs + s, fstat_aligned(xs), x);
    if (first_frame) {
      fstat_store<W>(fst + s, fstat_aligned(fst), x);
      fstat_store<W>(sum + s, fstat_aligned(sum), x);
#pragma unroll
      for (int i = 0; i < W; ++i) dev[v][i] = 0.;
    } else {
      fstat_load<W>(fst + s, fstat_aligned(fst), f);
      fstat_load<W>(sum + s, fstat_aligned(sum), t);
#pragma unroll
      for (int i = 0; i < W; ++i) { t[i] += x[i]; dev[v][i] = x[i] - f[i]; }
      fstat_store<W>(sum + s, fstat_aligned(sum), t);
    }
  }
  for (int p = 0; p < P.n; ++p) {
    double* __restrict__ pr = acc + (long long)(2 * NV + p) * n;
    double t[W];
    if (first_frame) {
#pragma unroll
      for (int i = 0; i < W; ++i) t[i] = 0.;
    } else {
      double da[W], db[W];
      fstat_pick<NV, W>(dev, P.a[p], da);
      fstat_pick<NV, W>(dev, P.b[p], db);
      fstat_load<W>(pr + s, fstat_aligned(pr), t);
#pragma unroll
      for (int i = 0; i < W; ++i) { const double q = da[i] * db[i]; t[i] += q; }   // the product first, then the sum
    }
    fstat_store<W>(pr + s, fstat_aligned(pr), t);
  }
}

// grid (blocks <= kMaxBlocks, 1, B), 256 threads.  Turn i of the grid takes the sites 2 i and 2 i + 1 of replica
// blockIdx.z; the last turn of an odd n is the scalar tail.  NV, the number of variables, is a template parameter: the
// deviations are a register array of exactly that size.
template <int NV>
__global__ void __launch_bounds__(256) k_fstat_accumulate(const double* __restrict__ src, long long src_rep, double* __restrict__ acc,
                                                          long long n, FstatVars V, FstatPairs P, int first_frame) {
  const double* __restrict__ mine = src + (long long)blockIdx.z * src_rep;
  double* __restrict__ into = acc + (long long)blockIdx.z * (2 * NV + P.n) * n;
  const long long turns = (n + 1) / 2, stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < turns; i += stride) {
    const long long s = 2 * i;
    if (s + 1 < n) fstat_sites<NV, 2>(mine, into, n, s, V, P, first_frame != 0);
    else fstat_sites<NV, 1>(mine, into, n, s, V, P, first_frame != 0);
  }
}

// what 1: mean of slot a; what 4: cov of the pair (a, b) with accumulator volume `pvol`; of replica `replica`, or,
// replica < 0, the ensemble value: the replicas added in the order 0 ... nrep-1 from 0, times inv_ens
__global__ void __launch_bounds__(256) k_fstat_derive(const double* __restrict__ acc, double* __restrict__ out, long long n, int nrep,
                                                      int nvars, int nvol, int what, int a, int b, int pvol, int replica,
                                                      double inv_n, double inv_ens) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const int r0 = replica < 0 ? 0 : replica, r1 = replica < 0 ? nrep : replica + 1;
  double ens = 0., one = 0.;
  for (int r = r0; r < r1; ++r) {
    const double* __restrict__ A = acc + (long long)r * nvol * n + s;
    if (what == 1) { one = A[(long long)a * n]; ens += one; one = one * inv_n; }
    else {
      const double ma = A[(long long)a * n] * inv_n, mb = A[(long long)b * n] * inv_n;
      const double da = ma - A[(long long)(nvars + a) * n], db = mb - A[(long long)(nvars + b) * n];
      const double shift = da * db;
      one = A[(long long)pvol * n] * inv_n - shift;
      ens += one;
    }
  }
  out[s] = replica < 0 ? ens * inv_ens : one;
}

int fstat_create(bflbm_ctx* c, bflbm_batch* b, bflbm_ring* g, int source, int nvars, const int* vars, int npairs,
                 const int* pair_a, const int* pair_b, int every, bflbm_fstat** out) {
  const char* call = b ? "bflbm_batch_fstat_create" : (g ? "bflbm_ring_fstat_create" : "bflbm_fstat_create");
  if (field_refuse_args(call, source, 2, nvars, vars, npairs, pair_a, pair_b)) return 1;
  if (every < 0) return fail("%s: every must be >= 0 (got %d)", call, every);
  if (store_refuse_owner(c, call, "bflbm_batch_fstat_create", "field statistic")) return 1;
  if (b && source == 2) return fail("%s: the observation of a batch has no noise form; source 2 needs a lone context or a ring", call);
  if (recorder_refuse_open(c, b, g, call)) return 1;
  const Geo& G = c ? c->G : (b ? b->G : g->ctx[0]->G);

  std::unique_ptr<bflbm_fstat> t(new bflbm_fstat());
  recorder_bind(t.get(), c, b, every, g);
  t->nx = G.nx; t->ny = G.ny; t->nz = G.nz;
  t->fs = field_select(b != nullptr, source, nvars, vars);
  t->pairs = field_pairs(npairs, pair_a, pair_b);

  const long long plane = (long long)G.nx * G.ny;
  if (g) {
    for (const bflbm_ctx* s : g->ctx) { FstatPart q; q.device = s->dom.device; q.z0 = s->dom.z0; q.n = (long long)s->nzl * plane; t->part.push_back(q); }
  } else {
    FstatPart q; q.device = t->device; q.z0 = 0; q.n = (long long)G.nz * plane; t->part.push_back(q);
  }
  const size_t fb = b ? (size_t)t->nrep * nvars * (size_t)t->part[0].n * sizeof(double) : 0;
  hipError_t e = hipSuccess;
  size_t ab = 0, ob = 0;
  for (FstatPart& q : t->part) {
    ab = (size_t)t->nrep * t->nvol() * (size_t)q.n * sizeof(double); ob = (size_t)q.n * sizeof(double);
    e = hipSetDevice(q.device);
    if (e == hipSuccess) e = hipMalloc((void**)&q.acc, ab);
    if (e == hipSuccess) e = hipMalloc((void**)&q.out, ob);
    if (e != hipSuccess) break;
  }
  if (e == hipSuccess && fb) { e = hipSetDevice(t->device); if (e == hipSuccess) e = hipMalloc((void**)&t->fields, fb); }
  if (e != hipSuccess) {                                     // the destructor frees what was allocated; no list was touched
    (void)hipGetLastError();
    return fail("%s: out of device memory (accumulators %zu + download %zu bytes per part of %zu, fields %zu): %s",
                call, ab, ob, t->part.size(), fb, hipGetErrorString(e));
  }
  recorder_list(t.get()).push_back(t.get());
  *out = t.release();
  return 0;
}

// the accumulation launch of one part on `stream`
int fstat_launch(const bflbm_fstat* t, const FstatPart& q, const double* src, long long src_rep, hipStream_t stream) {
  const long long turns = (q.n + 1) / 2;
  const unsigned blocks = (unsigned)std::min<long long>((turns + 255) / 256, fstat_limits::kMaxBlocks);
  const dim3 grid(blocks, 1, (unsigned)t->nrep);
  const int first_frame = t->n == 0 ? 1 : 0;
  if (!field_dispatch_nv(t->fs.nvars, [&](auto nv) {
        hipLaunchKernelGGL((k_fstat_accumulate<decltype(nv)::value>), grid, dim3(256), 0, stream, src, src_rep, q.acc, q.n, t->fs.vol, t->pairs, first_frame);
      })) return fail("field statistic: %d variables", t->fs.nvars);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace

// enqueue the observation and the accumulation of the resident state as frame n; no host synchronisation
int bflbm_fstat::record() {
  const char* asker = "field statistics sample";
  const double* dense;
  long long rep_stride;
  if (!ring) {
    if (fields_observe(this, fs, fields, asker, &dense, &rep_stride)) return 1;
    if (fstat_launch(this, part[0], dense, rep_stride, recorder_stream(this))) return 1;
  } else {
    if (fs.source != 1 && ring_prepare_ref(ring)) return 1; // the global centre of mass: the slabs' own prepare_ref is then a no-op
    for (size_t k = 0; k < part.size(); ++k) {
      bflbm_ctx* c = ring->ctx[k];
      if (fields_observe_slab(c, fs, asker, &dense)) return 1;
      if (fstat_launch(this, part[k], dense, 0, c->stream)) return 1;
    }
  }
  n += 1;
  return 0;
}

extern "C" {

int bflbm_fstat_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                       int every, bflbm_fstat** out) {
  if (!c || !vars || !out) return fail("bflbm_fstat_create: null argument");
  return fstat_create(c, nullptr, nullptr, source, nvars, vars, npairs, pair_a, pair_b, every, out);
}
int bflbm_batch_fstat_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                             int every, bflbm_fstat** out) {
  if (!b || !vars || !out) return fail("bflbm_batch_fstat_create: null argument");
  return fstat_create(nullptr, b, nullptr, source, nvars, vars, npairs, pair_a, pair_b, every, out);
}
int bflbm_ring_fstat_create(bflbm_ring* r, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                            int every, bflbm_fstat** out) {
  if (!r || !vars || !out) return fail("bflbm_ring_fstat_create: null argument");
  if (r->ctx.size() == 1)                                  // the whole box: the lone recorder of ctx[0], served by its steps
    return fstat_create(r->ctx[0], nullptr, nullptr, source, nvars, vars, npairs, pair_a, pair_b, every, out);
  return fstat_create(nullptr, nullptr, r, source, nvars, vars, npairs, pair_a, pair_b, every, out);
}

int bflbm_fstat_destroy(bflbm_fstat* s) {
  if (!s) return 0;
  recorder_detach(s);                                      // waits for the frames in flight: they write the buffers freed below
  delete s;
  return 0;
}

int bflbm_fstat_sample(bflbm_fstat* s) {
  if (!s) return fail("bflbm_fstat_sample: null argument");
  if (!recorder_attached(s)) return fail("bflbm_fstat_sample: the owner of the field statistic was destroyed");
  if (recorder_owner_open(s)) return fail("bflbm_fstat_sample inside an open step");
  return s->record();
}

int bflbm_fstat_reset(bflbm_fstat* s) {                    // frame 0 writes every accumulator: nothing to zero
  if (!s) return fail("bflbm_fstat_reset: null argument");
  if (recorder_owner_open(s)) return fail("bflbm_fstat_reset inside an open step");
  s->n = 0; s->since = 0;
  return 0;
}

int bflbm_fstat_count(const bflbm_fstat* s, long long* nsamples, int* nreplicas) {
  if (!s) return fail("bflbm_fstat_count: null argument");
  if (nsamples) *nsamples = s->n;
  if (nreplicas) *nreplicas = s->nrep;
  return 0;
}

int bflbm_fstat_get(bflbm_fstat* s, int what, int index, int replica, double* dst) {
  if (!s || !dst) return fail("bflbm_fstat_get: null argument");
  if (what < 0 || what > 4) return fail("bflbm_fstat_get: what must be 0 (sum), 1 (mean), 2 (first), 3 (prod) or 4 (cov) (got %d)", what);
  const bool of_pair = what >= 3;
  const int most = of_pair ? s->pairs.n : s->fs.nvars;
  if (index < 0 || index >= most) return fail("bflbm_fstat_get: %s %d of %d", of_pair ? "pair" : "variable slot", index, most);
  if (replica < -1 || replica >= s->nrep) return fail("bflbm_fstat_get: replica %d of %d (-1: the ensemble value)", replica, s->nrep);
  if (replica < 0 && what != 1 && what != 4) return fail("bflbm_fstat_get: only mean (1) and cov (4) have an ensemble value (what = %d)", what);
  if (s->n == 0) return fail("bflbm_fstat_get: no frame was taken yet");
  if (recorder_owner_open(s)) return fail("bflbm_fstat_get inside an open step");
  const int nv = s->fs.nvars, nvol = s->nvol();
  const double inv_n = 1.0 / (double)s->n;
  const double inv_ens = what == 1 ? 1.0 / ((double)s->nrep * (double)s->n) : 1.0 / (double)s->nrep;
  const int a = of_pair ? s->pairs.a[index] : index, b = of_pair ? s->pairs.b[index] : index;
  const int raw_vol = what == 0 ? index : (what == 2 ? nv + index : 2 * nv + index);
  const long long plane = (long long)s->nx * s->ny;
  for (size_t k = 0; k < s->part.size(); ++k) {
    const FstatPart& q = s->part[k];
    HIP_TRY(hipSetDevice(q.device));
    // detaching waited for everything enqueued: plain copies then
    const bool live = recorder_attached(s);
    const hipStream_t stream = !live ? nullptr : (s->ctx ? s->ctx->stream : (s->batch ? s->batch->stream : s->ring->ctx[k]->stream));
    const double* from;
    if (what == 1 || what == 4) {
      hipLaunchKernelGGL(k_fstat_derive, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, stream, q.acc, q.out, q.n, s->nrep,
                         nv, nvol, what, a, b, 2 * nv + index, replica, inv_n, inv_ens);
      HIP_TRY(hipGetLastError());
      from = q.out;
    } else {
      from = q.acc + ((long long)replica * nvol + raw_vol) * q.n;
    }
    HIP_TRY(hipMemcpyAsync(dst + (long long)q.z0 * plane, from, (size_t)q.n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return 0;
}

}  // extern "C"

#endif  // BFLBM_FSTAT_H_
