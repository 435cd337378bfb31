// bflbm_recorder.h -- the one lifecycle of everything that records from an owner's resident state: ensemble traces
// (bflbm_trace.h), interface traces (bflbm_iface.h), shape traces (bflbm_shape.h), structure factors (bflbm_sf.h,
// bflbm_sf_ring.h, bflbm_batch_sf.h), spectrum traces (bflbm_spectrum.h, bflbm_spectrum_ring.h), mode traces (bflbm_modes.h), field
// statistics (bflbm_fstat.h), profile traces (bflbm_profile.h), histogram traces (bflbm_hist.h), morphology traces
// (bflbm_morph.h), chord traces (bflbm_chord.h), coarse traces (bflbm_coarse.h), lag traces (bflbm_lag.h), moment traces (bflbm_moment.h), cluster traces (bflbm_cluster.h), component traces (bflbm_components.h) and radial traces (bflbm_radial.h).  A recorder is attached to a lone context, a batch or a ring of more than one slab, is served after
// every step on the owner's stream(s) in creation order, survives its owner detached (readable, no longer fed) and is
// destroyed by its own call ("Recorders").  A ring serves its recorders from bflbm_ring_step only, after the
// bflbm_step_finish of every slab; its samples carry slab 0's step counter and its records live on slab 0's device,
// written on slab 0's stream (field statistics excepted: a per-site accumulator stays on the slab that owns the site).
// Below the lifecycle, two things the kinds share: the sample store of every kind but the two accumulators (structure
// factors, field statistics), which owns its records and its stage buffer, and the ring gather, by which the kinds that
// reduce on every slab of a ring (moments, profile, histogram and spectrum traces) bring one block per slab to slab 0.
// The layer above it, what the kinds that read observed fields share, is bflbm_fieldsel.h.
// Host code only.  Included by bflbm.hip once bflbm_ctx, bflbm_batch and bflbm_ring are complete (needs fail, HIP_TRY).
#ifndef BFLBM_RECORDER_H_
#define BFLBM_RECORDER_H_

struct bflbm_recorder {
  bflbm_ctx* ctx = nullptr;        // the owner: a lone context ...
  bflbm_batch* batch = nullptr;    // ... or a batch ...
  bflbm_ring* ring = nullptr;      // ... or a ring of more than one slab; all null once the owner is gone (detached)
  int device = 0;
  int nrep = 1;
  int every = 0;                   // a sample after every `every`-th step through the owner; 0: stepping never serves it
  long long since = 0;             // steps taken through the owner since creation or reset
  long long n = 0;                 // samples (frames) recorded
  long long capacity = std::numeric_limits<long long>::max();   // unbounded: an accumulator
  std::vector<long long> steps;    // [n][nrep]: every replica's step counter at the sample
  const char* const noun;          // "trace", "interface trace": the messages
  const char* const abi;           // "bflbm_trace", "bflbm_iface": the calls the messages name
  bflbm_recorder(const char* noun_, const char* abi_) : noun(noun_), abi(abi_) {}
  virtual ~bflbm_recorder() {}
  virtual int record() = 0;        // enqueue one sample (frame) of the resident state now; no host synchronisation
};

// what the trace kinds add: `capacity` samples of `per` doubles on the device, and a stage buffer of the kind's own.
// The store owns both: store_attach allocates them, the destructor frees them.
struct bflbm_sample_store : bflbm_recorder {
  using bflbm_recorder::bflbm_recorder;
  size_t per = 0;
  double* d_rec = nullptr;         // [capacity][per]
  double* d_stage = nullptr;       // stage 1 -> stage 2
  ~bflbm_sample_store() override {
    if (!d_rec && !d_stage) return;
    hipSetDevice(device);
    if (d_rec) hipFree(d_rec);
    if (d_stage) hipFree(d_stage);
  }
};

// The ring gather: how a kind that reduces on every slab of a ring brings one block per slab to slab 0 (DESIGN.md,
// "Recorders").  Slab k > 0 writes its block on its own device and stream and records `done`; slab 0's stream waits for
// every `done`, copies each block to its place in a buffer of slab 0 and records `taken`; before slab k overwrites its
// block for the next sample its stream waits for `taken`.  Empty unless the owner is a ring of more than one slab.
struct RingGather {
  struct Part { int device = 0; void* block = nullptr; size_t bytes = 0, at = 0; hipEvent_t done = nullptr; };   // slab k > 0; part[0] stays empty
  std::vector<Part> part;
  int device = 0;                  // slab 0's
  hipEvent_t taken = nullptr;      // slab 0 has copied every slab's block of the last sample
  RingGather() = default;
  RingGather(const RingGather&) = delete;
  RingGather& operator=(const RingGather&) = delete;
  ~RingGather() {
    for (Part& q : part) {
      if (!q.block && !q.done) continue;
      hipSetDevice(q.device);
      if (q.block) hipFree(q.block);
      if (q.done) hipEventDestroy(q.done);
    }
    if (taken) { hipSetDevice(device); hipEventDestroy(taken); }
  }
};

namespace {

inline bool recorder_attached(const bflbm_recorder* r) { return r->ctx || r->batch || r->ring; }
// the stream that writes the records: a ring's is slab 0's
inline hipStream_t recorder_stream(const bflbm_recorder* r) { return r->ctx ? r->ctx->stream : (r->batch ? r->batch->stream : r->ring->ctx[0]->stream); }
inline bool ring_step_open(const bflbm_ring* g) { for (const bflbm_ctx* c : g->ctx) if (c->step_open()) return true; return false; }
inline bool recorder_owner_open(const bflbm_recorder* r) { return (r->ctx && r->ctx->step_open()) || (r->ring && ring_step_open(r->ring)); }
inline std::vector<bflbm_recorder*>& recorder_list(bflbm_recorder* r) { return r->ctx ? r->ctx->recorders : (r->batch ? r->batch->recorders : r->ring->recorders); }

// samples that `nsteps` more steps through the owner add
inline long long recorder_due(const bflbm_recorder* r, long long nsteps) { return r->every ? (r->since + nsteps) / r->every - r->since / r->every : 0; }
inline bool recorder_overflows(const bflbm_recorder* r, long long nsteps) { return recorder_due(r, nsteps) > r->capacity - r->n; }

// the link to the owner; the owner's list takes the recorder once nothing can fail any more
void recorder_bind(bflbm_recorder* r, bflbm_ctx* c, bflbm_batch* b, int every, bflbm_ring* g = nullptr) {
  r->ctx = c; r->batch = b; r->ring = g; r->every = every;
  r->device = c ? c->dom.device : (b ? b->device : g->ctx[0]->dom.device);
  r->nrep = b ? (int)b->ctx.size() : 1;
}

int recorder_after_step(bflbm_recorder* r) {
  r->since += 1;
  return (r->every && r->since % r->every == 0) ? r->record() : 0;
}

// the owner goes away (or the recorder does): what was enqueued completes, what was recorded stays readable
void recorder_detach(bflbm_recorder* r) {
  if (!recorder_attached(r)) return;
  if (r->ring) {                                       // a sample runs on every slab's stream
    for (const bflbm_ctx* c : r->ring->ctx) { hipSetDevice(c->dom.device); (void)hipStreamSynchronize(c->stream); }
  } else {
    hipSetDevice(r->device);
    (void)hipStreamSynchronize(recorder_stream(r));
  }
  std::vector<bflbm_recorder*>& list = recorder_list(r);
  list.erase(std::remove(list.begin(), list.end(), r), list.end());
  r->ctx = nullptr; r->batch = nullptr; r->ring = nullptr;
}

// ---- the owner's side: a bflbm_ctx, a bflbm_batch or a bflbm_ring with its `recorders` in creation order -------------------------------
template <class Owner> void recorders_detach_all(Owner* o) { while (!o->recorders.empty()) recorder_detach(o->recorders.back()); }

// a call of `nsteps` steps is refused before any launch when some recorder's samples would not fit
template <class Owner> int recorders_refuse_full(const Owner* o, const char* call, long long nsteps) {
  for (const bflbm_recorder* r : o->recorders)
    if (recorder_overflows(r, nsteps))
      return fail("%s: %s full: the samples of %lld more step(s) do not fit (read it and %s_reset, or create a larger one)", call, r->noun, nsteps, r->abi);
  return 0;
}

// one step was taken through the owner
template <class Owner> int recorders_after_step(Owner* o) {
  for (bflbm_recorder* r : o->recorders) if (recorder_after_step(r)) return 1;
  return 0;
}

// ---- the ring gather -----------------------------------------------------------------------------------------------------
// The events of every slab k > 0 and its block of bytes_of(k) bytes, which lands at byte at_of(k) of the destination.
// On failure the gather holds only what its destructor frees.  Leaves the last slab's device selected.
template <class BytesOf, class AtOf>
hipError_t gather_create(RingGather& G, const bflbm_ring* g, BytesOf bytes_of, AtOf at_of) {
  G.device = g->ctx[0]->dom.device;
  G.part.resize(g->ctx.size());
  hipError_t e = hipSetDevice(G.device);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&G.taken, hipEventDisableTiming);
  for (int k = 1; k < (int)G.part.size() && e == hipSuccess; ++k) {
    RingGather::Part& q = G.part[k];
    q.device = g->ctx[k]->dom.device; q.bytes = bytes_of(k); q.at = at_of(k);
    e = hipSetDevice(q.device);
    if (e == hipSuccess) e = hipMalloc(&q.block, q.bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&q.done, hipEventDisableTiming);
  }
  return e;
}
// where slab k's launch writes: its block, or slab 0's own place in the destination
template <class T> inline T* gather_target(const RingGather& G, int k, T* own) { return k > 0 ? static_cast<T*>(G.part[k].block) : own; }
// Around the launch on slab k's stream that overwrites its block (slab 0 has none: both do nothing).  hold: slab 0 may
// still be copying the last sample's block; a `taken` never recorded (the first sample) is complete, the wait a no-op.
int gather_hold(const RingGather& G, int k, hipStream_t stream) {
  if (k > 0) HIP_TRY(hipStreamWaitEvent(stream, G.taken, 0));
  return 0;
}
int gather_ready(const RingGather& G, int k, hipStream_t stream) {
  if (k > 0) HIP_TRY(hipEventRecord(G.part[k].done, stream));
  return 0;
}
// on slab 0's stream, its device selected: every block to its place in dst, in slab order
int gather_take(const RingGather& G, void* dst, hipStream_t s0) {
  for (size_t k = 1; k < G.part.size(); ++k) {
    const RingGather::Part& q = G.part[k];
    HIP_TRY(hipStreamWaitEvent(s0, q.done, 0));
    HIP_TRY(hipMemcpyPeerAsync(static_cast<char*>(dst) + q.at, G.device, q.block, q.device, q.bytes, s0));
  }
  HIP_TRY(hipEventRecord(G.taken, s0));
  return 0;
}

// ---- the sample store ------------------------------------------------------------------------------------------------------
int store_refuse_cadence(const char* call, int every, long long capacity) {
  if (every < 1) return fail("%s: every must be >= 1 (got %d)", call, every);
  if (capacity < 1) return fail("%s: capacity must be >= 1 (got %lld)", call, capacity);
  return 0;
}
// `batch_call`: the creation call of the kind that takes a batch; `noun`: the kind's, as in its messages
int store_refuse_owner(const bflbm_ctx* c, const char* call, const char* batch_call, const char* noun) {
  if (c && c->batch) return fail("%s: the context is a replica of a batch; use %s on the batch", call, batch_call);
  if (c && !c->G.zwrap) return fail("%s: a slab of a decomposed lattice (nranks > 1); %ss take a lone single-slab context or a batch", call, noun);
  return 0;
}

// `capacity` samples of `per` 8-byte words for `nrep` replicas; `shape`: what besides the replicas multiplies the
// capacity, for the message.  store_attach asks; a kind that allocates much of its own before it asks first.
int store_refuse_capacity(const char* call, long long capacity, size_t per, int nrep, const char* shape) {
  if ((unsigned long long)capacity > ((1ULL << 40) / sizeof(double)) / per)
    return fail("%s: capacity %lld x %d replicas%s exceeds 1 TB of records", call, capacity, nrep, shape);
  return 0;
}

// allocate [capacity][per] and the stage buffer and attach the store to its owner.  The last step of a creation call:
// the owner's list has the store afterwards, so what can fail comes before it (or detaches again).  On failure the
// store's destructor frees what was allocated.
int store_attach(bflbm_sample_store* s, bflbm_ctx* c, bflbm_batch* b, const char* call, int every, long long capacity,
                 size_t per, size_t stage_doubles, const char* shape, bflbm_ring* g = nullptr) {
  if ((c && c->step_open()) || (g && ring_step_open(g))) return fail("%s inside an open step", call);
  recorder_bind(s, c, b, every, g);
  if (store_refuse_capacity(call, capacity, per, s->nrep, shape)) return 1;
  HIP_TRY(hipSetDevice(s->device));
  hipError_t e = hipMalloc((void**)&s->d_rec, (size_t)capacity * per * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_stage, stage_doubles * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail("%s: %s", call, hipGetErrorString(e));
  }
  s->capacity = capacity; s->per = per;
  recorder_list(s).push_back(s);
  return 0;
}

// the head and the tail of a kind's record(): refuse a full store and select the device; the slot of sample n; count
// the sample under every replica's step counter
int store_begin(const bflbm_sample_store* s) {
  if (s->n >= s->capacity) return fail("%s full: %lld samples recorded (read it and %s_reset, or create a larger one)", s->noun, s->n, s->abi);
  HIP_TRY(hipSetDevice(s->device));
  return 0;
}
inline double* store_slot(const bflbm_sample_store* s) { return s->d_rec + (size_t)s->n * s->per; }
void store_recorded(bflbm_sample_store* s) {
  if (s->batch) for (const bflbm_ctx* c : s->batch->ctx) s->steps.push_back(c->steps);
  else s->steps.push_back(s->ctx ? s->ctx->steps : s->ring->ctx[0]->steps);
  s->n += 1;
}

int store_destroy(bflbm_sample_store* s) {
  if (!s) return 0;
  recorder_detach(s);                                  // waits for the work in flight: it writes the buffers the destructors free
  hipSetDevice(s->device);                             // a kind's destructor frees its lone and batch buffers on the selected device
  delete s;
  return 0;
}

// `abi` below: the kind's prefix again, for the refusal of a null store, which has no abi field to read
int store_sample(bflbm_sample_store* s, const char* abi) {
  if (!s) return fail("%s_sample: null argument", abi);
  if (!recorder_attached(s)) return fail("%s_sample: the owner of the %s was destroyed", abi, s->noun);
  if (recorder_owner_open(s)) return fail("%s_sample inside an open step", abi);
  return s->record();
}

int store_reset(bflbm_sample_store* s, const char* abi) {
  if (!s) return fail("%s_reset: null argument", abi);
  if (recorder_owner_open(s)) return fail("%s_reset inside an open step", abi);
  s->n = 0; s->since = 0;
  s->steps.clear();
  return 0;
}

int store_count(const bflbm_sample_store* s, const char* abi, long long* nsamples, int* nreplicas) {
  if (!s) return fail("%s_count: null argument", abi);
  if (nsamples) *nsamples = s->n;
  if (nreplicas) *nreplicas = s->nrep;
  return 0;
}

int store_read(bflbm_sample_store* s, const char* abi, long long first, long long count, double* rec, long long* steps) {
  if (!s) return fail("%s_read: null argument", abi);
  if (first < 0 || count < 0 || first > s->n || count > s->n - first)
    return fail("%s_read: samples [%lld, %lld + %lld) of %lld recorded", abi, first, first, count, s->n);
  if (count == 0) return 0;
  if (!rec) return fail("%s_read: null argument", abi);
  if (recorder_owner_open(s)) return fail("%s_read inside an open step", abi);
  HIP_TRY(hipSetDevice(s->device));
  const double* src = s->d_rec + (size_t)first * s->per;
  const size_t nb = (size_t)count * s->per * sizeof(double);
  if (recorder_attached(s)) {
    const hipStream_t stream = recorder_stream(s);
    HIP_TRY(hipMemcpyAsync(rec, src, nb, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  } else {
    HIP_TRY(hipMemcpy(rec, src, nb, hipMemcpyDeviceToHost));   // detaching waited for everything enqueued
  }
  if (steps) std::copy(s->steps.begin() + (size_t)first * s->nrep, s->steps.begin() + (size_t)(first + count) * s->nrep, steps);
  return 0;
}

}  // namespace

#endif  // BFLBM_RECORDER_H_
