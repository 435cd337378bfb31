/*
 * bflbm.h -- C-ABI of the MI355X-native D3Q19 binary fluctuating-LBM hot path.
 *
 * The reference (MDProject/Binary-Fluctuating-Lattice-Boltzmann) has no FFI layer:
 * its operator surface is a set of C++ free functions over AMReX MultiFabs
 * (LBM_binary.H).  Each entry point below names the reference interface it
 * replaces.  The header adapter include/bflbm_amrex.H re-creates those C++
 * signatures on top of this ABI; python binds it with ctypes.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; the message is
 *    available from bflbm_last_error() (the reference returns void and aborts,
 *    LBM_binary.H:622 AMREX_GPU_ERROR_CHECK / Debug.H:141 exit).
 *  - host arrays use the AMReX FAB layout: x fastest, then y, z, component
 *    slowest, over a box [lo,hi] that may include ghost cells (bflbm_fab).
 *  - one context = one z-slab [z0,z1) of a periodic nx*ny*nz lattice on one
 *    GPU.  Work is enqueued on the context's HIP stream; call bflbm_sync()
 *    (or synchronise the stream you supplied) before reading results.
 *  - not re-entrant per context; one host thread per context.
 */
#ifndef BFLBM_H_
#define BFLBM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFLBM_NVEL 19          /* nvel, LBM_d3q19.H:4 */
#define BFLBM_NHYDRO 22        /* hydrovs components, main_run_job.cpp:147 */
#define BFLBM_NHYDROBAR 9      /* hydrovsbar components actually defined, LBM_binary.H:329-339 */
#define BFLBM_ABI_VERSION 1

/* Mirrors the reference's process-wide model globals.
 * tau_f,tau_g,alpha0,alpha1,kappa,seed: LBM_binary.H:17-30; kBT,cs2: LBM_d3q19.H:6-10;
 * rho_lo,rho_hi: LBM_binary.H:25-26.  alpha1 is carried but unused (LBM_binary.H:256-257). */
typedef struct bflbm_params {
  double tau_f, tau_g;
  double alpha0, alpha1;
  double kappa;
  double kBT;
  double cs2;
  double rho_lo, rho_hi;
  uint64_t seed;
} bflbm_params;

/* Lattice and slab.  Replaces Geometry/BoxArray/DistributionMapping of
 * main_run_job.cpp:136-143 for the path: periodic box, z-slab per GPU. */
typedef struct bflbm_domain {
  int n[3];       /* global lattice nx,ny,nz */
  int z0, z1;     /* this context owns global planes z0 <= z < z1 */
  int rank;       /* slab index 0..nranks-1 (ring neighbours rank+-1 mod nranks) */
  int nranks;     /* 1: z wraps inside the context, no halo exchange needed */
  int device;     /* HIP device ordinal */
} bflbm_domain;

/* A host array in AMReX FAB layout: allocated over cells lo..hi inclusive (global
 * indices, ghost cells included, this fixes the strides); only the cells of the
 * valid region vlo..vhi that lie inside the context's slab are read or written
 * (MFIter::validbox semantics, e.g. LBM_binary.H:609). */
typedef struct bflbm_fab {
  int lo[3];
  int hi[3];
  int vlo[3];
  int vhi[3];
} bflbm_fab;

typedef struct bflbm_ctx bflbm_ctx;

/* Fill *p with the reference's shipped defaults (LBM_binary.H:17-30, LBM_d3q19.H:6-10). */
void bflbm_default_params(bflbm_params* p);

int bflbm_abi_version(void);
const char* bflbm_last_error(void);

/* Number of HIP devices visible (does not create a context). */
int bflbm_device_count(int* n);

/* Allocate the resident state (two A/B buffers of 2x19 populations + rho/phi). */
int bflbm_create(const bflbm_params* p, const bflbm_domain* d, bflbm_ctx** out);
int bflbm_destroy(bflbm_ctx* c);

/* The reference edits its globals between runs (ReadMe.ipynb cells 1-3). */
int bflbm_set_params(bflbm_ctx* c, const bflbm_params* p);
int bflbm_get_params(const bflbm_ctx* c, bflbm_params* p);

/* external != 0: enqueue all work on the caller's hipStream_t (e.g. torch's current stream; the
 * handle may be NULL = the legacy default stream, which is what torch uses by default).
 * external == 0: go back to the context's own non-blocking stream (hip_stream ignored). */
int bflbm_set_stream(bflbm_ctx* c, void* hip_stream, int external);

/* Kernel schedule (what one LBM_timestep, LBM_binary.H:545-594, is run as):
 *   0  two-pass (density pass + collide pass); bit-exact; the only one that takes injected or reference-state noise
 *   1  fused plane-marching kernel, tile-ring densities pulled; bit-exact; zero noise or generated noise
 *   3  pipelined plane-marching kernel, tile-ring densities handed over from the previous step
 *      (csrc/bflbm_handover.h); zero noise or generated thermal noise (it draws the normals itself); takes every lattice
 *      with nx >= 64, ny >= 4, nx % 64 != 1, ny % 4 != 1 (a narrower last tile column and a lower last tile row are
 *      handled) and no injected noise, otherwise it resolves to the bit-exact schedule (1 at zero noise, 0 with noise).
 *      Fails if its frames (5.6 % of the state) cannot be allocated.
 *   2  auto (default): 3 where it applies AND is the faster kernel (marches of >= 16 planes; at zero noise a last tile
 *      column with >= 77 % of its lanes busy) AND alpha0 x (total density) <= 6, the total density rho + phi being
 *      |rho_hi| + |rho_lo| after an analytic init and the largest |rho + phi| of the uploaded state after LBM_init
 *      (bflbm_state_total_max), AND the frames fit in device memory;
 *      else a bit-exact schedule: 0 with noise, and at zero noise 1, or 0 on lattices too small to give the one-pass kernel
 *      a workgroup per CU.  BFLBM_AUTO_EXACT=1 in the environment keeps auto bit-exact, with and without noise.
 * Schedules 0 and 1 give the CPU reference's doubles (same operation order).  Schedule 3 adds the 19 populations of a
 * tile-ring density in another fixed order: deterministic and run-to-run reproducible.  Its contract (the same
 * sentence in DESIGN.md, INTEGRATION.md and README.md; one test per clause in tests/test_gpu_handover_oracle.py): the
 * first step after an init or upload equals the CPU reference path bit for bit; after that the results differ from it
 * by what a one-ulp change of the reference's own state does: in a well-conditioned run rho, phi, rho + phi agree to
 * 1e-12 relative and the velocities to 1e-12 max(cs, |u|) absolute at every site, except at near-vacuum sites (a
 * density below 1e-3 of its field's maximum), where the bound holds for the density relative to the field maximum and
 * for the momentum; in a run through a violent transient (spinodal demixing: velocities of thousands of lattice units
 * at near-vacuum sites) the difference is bounded by that run's own one-ulp response and by nothing smaller.  Of the
 * 92 oracle comparisons of the test suite 75 meet the strict form at every site; the others are listed with their
 * unmasked maxima in tests/golden/handover_strict_exceptions.json and held to 10 x the oracle's own one-ulp response,
 * and so is a demixing mixture (alpha0 = 2.5, kBT = 1e-5), whose one-ulp response reaches 1e-9 of the densities and
 * 5e-3 cs in the velocities within 100 steps. Where the reference run itself diverges (interaction strength alpha0 x
 * total density >= 7.5: NaN on the CPU path within tens of steps) nothing bounds the difference -- hence the parameter
 * bound in auto. */
int bflbm_set_schedule(bflbm_ctx* c, int schedule);
/* The schedule (0, 1 or 3) the next step of this context will run with its current parameters and lattice. */
int bflbm_resolved_schedule(const bflbm_ctx* c, int* schedule);

/* LBM_init_mixture (LBM_binary.H:598-629), LBM_init_stripe(frac) (:664-695),
 * LBM_init_droplet(r) (:699-742).  Resets the step counter to 0. */
int bflbm_init_mixture(bflbm_ctx* c);
int bflbm_init_stripe(bflbm_ctx* c, double frac);
int bflbm_init_droplet(bflbm_ctx* c, double r);

/* LBM_init from given populations (LBM_binary.H:632-661 / mf.ParallelCopy(mf0)):
 * copy the cells of `box` that lie in the slab from host arrays f,g (19 comps each).
 * Call once per box of a multi-box MultiFab, then bflbm_commit_upload(). */
int bflbm_upload_fg(bflbm_ctx* c, const double* f, const double* g, const bflbm_fab* box);
int bflbm_commit_upload(bflbm_ctx* c, int reset_step_counter);
/* The total density `auto` keys its stability bound on (bflbm_set_schedule): the largest |rho + phi| of the state the last
 * bflbm_commit_upload made resident (LBM_init, LBM_binary.H:632-661); 2 after LBM_init_mixture (rho = phi = 1 at every site,
 * :613-614); a negative number after LBM_init_stripe / _droplet (then rho_hi + rho_lo of the parameters is that number at every site).  A driver that owns several slabs hands each slab the
 * maximum over all of them (bflbm_ring_commit_upload does). */
int bflbm_state_total_max(const bflbm_ctx* c, double* total_max);
int bflbm_set_state_total_max(bflbm_ctx* c, double total_max);

/* fold/gold valid cells after LBM_timestep (state t): write the slab's cells
 * that lie inside `box` into f,g (ghost cells of the destination are not touched). */
int bflbm_download_fg(bflbm_ctx* c, double* f, double* g, const bflbm_fab* box);

/* LBM_timestep (LBM_binary.H:545-594) applied nsteps times.  For nranks > 1 the
 * caller must run the halo exchange between steps (see bflbm_halo_*), so only
 * nsteps == 1 is accepted there; python/ C++ drivers wrap this. */
int bflbm_step(bflbm_ctx* c, int nsteps);
int bflbm_step_count(const bflbm_ctx* c, long long* steps_done);
/* The step counter is also the noise index of the counter-based generator (one fresh set of 33 normals per site and
 * index).  A run continued from a kBT > 0 checkpoint (main_run_job.cpp:80 step_continue, :253-270) sets it to the
 * checkpoint's absolute step after bflbm_commit_upload(c, 1), so that it does not replay the first segment's normals.
 * The counter is 64 bits wide and keeps counting; the noise index is the counter modulo 2^32, so the step after counter
 * 2^32 - 1 draws index 0 again while bflbm_step_count reports 2^32.  Moving the counter changes the generated noise of
 * the resident state (and what bflbm_get_noise / bflbm_get_hydrovs return), nothing else. */
int bflbm_set_step_count(bflbm_ctx* c, long long steps_done);

/* One step of a slab (nranks > 1) split so that the +-z exchange overlaps the
 * interior planes.  Precondition: the resident state has valid halo planes.
 *   bflbm_step_boundary  -> the two outermost plane pairs of the slab
 *   bflbm_halo_pack(BFLBM_HALO_NEXT, side, buf) for side 0,1; start the exchange
 *   bflbm_step_interior  -> all other planes (overlaps the exchange)
 *   wait; bflbm_halo_unpack(BFLBM_HALO_NEXT, side, buf)
 *   bflbm_step_finish    -> swap A/B buffers, advance the step counter
 * With nranks == 1 these also work (halo calls are then not needed).
 * The step is open from bflbm_step_boundary to bflbm_step_finish and runs the schedule bflbm_step_boundary resolved with the
 * parameters it had then: inside it bflbm_set_params, bflbm_set_schedule, bflbm_inject_noise, bflbm_set_state_total_max,
 * bflbm_set_ref_state, bflbm_enable_ref_state, bflbm_set_com, bflbm_set_step_count, bflbm_tune_placement, downloads,
 * observables and reductions are refused ("... inside an open step").  A failed bflbm_step_boundary or
 * bflbm_step_interior closes the step with the resident state intact: it may be retried, on another schedule too. */
int bflbm_step_boundary(bflbm_ctx* c);
int bflbm_step_interior(bflbm_ctx* c);
int bflbm_step_finish(bflbm_ctx* c);

/* Halo exchange support (replaces the +-z part of fold/gold/hydrovs FillBoundary,
 * LBM_binary.H:553-555; x,y wrap inside the slab).  side 0 = low-z face, 1 = high-z
 * face.  pack: gather what the neighbour on that side needs into a contiguous
 * device buffer; unpack: store what was received FROM the neighbour on that side.
 * kind selects the buffer and the plane set. */
#define BFLBM_HALO_STATE 0   /* resident post-collision state: 38 component-planes per side */
#define BFLBM_HALO_NEXT 1    /* same set, on the buffer the open step is writing */
#define BFLBM_HALO_UPLOAD 2  /* uploaded populations before bflbm_commit_upload: 38 comps x 1 plane */
int bflbm_halo_bytes(const bflbm_ctx* c, int kind, size_t* bytes_per_side);
int bflbm_halo_pack(bflbm_ctx* c, int kind, int side, void* device_buf);
int bflbm_halo_unpack(bflbm_ctx* c, int kind, int side, const void* device_buf);
/* The same exchange WITHOUT staging: entry k of the face (k < *count = 38) is one contiguous component plane of
 * *plane_bytes bytes at planes[k] in device memory -- pack != 0: where this slab's boundary planes hold what the neighbour
 * across `side` needs; pack == 0: the halo plane on `side` that receives it (entry k of a sender's face pairs with entry
 * k of the receiver's opposite face).  The addresses are those of the state buffer `kind` names at the time of the call
 * (they alternate from step to step).  A transport that can post 38 sends per face (RCCL group, peer copies) needs no
 * pack/unpack kernels and no buffers; bflbm_halo_pack/_unpack remain for transports that want one message per face.
 * Replaces the same FillBoundary calls (LBM_binary.H:553-555). */
int bflbm_halo_planes(bflbm_ctx* c, int kind, int side, int pack, void** planes, size_t* plane_bytes, int* count);

/* ---- Single-process ring of slabs (the reference runs as ONE process, USE_MPI=FALSE, GNUmakefile:16):
 * nslabs z-slabs of one lattice, slab r on GPU devices[r % ndevices]; the +-z exchange of every step is
 * done with device-to-device (peer, xGMI) copies on a second stream per slab and overlaps the interior
 * planes.  nslabs == 1 is the plain single-GPU case.  Per-slab work (upload, download, observables,
 * noise injection) goes through the slab's context from bflbm_ring_slab(); every bflbm_get_* /
 * bflbm_upload_fg / bflbm_download_fg call only touches the cells of the given box that lie in that slab,
 * so a driver simply loops over the slabs.  This is what include/bflbm_amrex.H drives.
 * A ring of more than one slab may own recorders (bflbm_ring_trace_create, bflbm_ring_spectrum_create below):
 * bflbm_ring_step refuses a call whose samples would not fit before any launch and serves the recorders once per step,
 * after the bflbm_step_finish of every slab.  Stepping the slabs by hand through bflbm_ring_slab() serves nothing.
 * bflbm_ring_destroy detaches the ring's recorders first; they stay readable. */
typedef struct bflbm_ring bflbm_ring;
int bflbm_ring_create(const bflbm_params* p, const int n[3], int nslabs, const int* devices, int ndevices, bflbm_ring** out);
int bflbm_ring_destroy(bflbm_ring* r);
int bflbm_ring_size(const bflbm_ring* r, int* nslabs);
int bflbm_ring_slab(bflbm_ring* r, int slab, bflbm_ctx** ctx);
int bflbm_ring_set_params(bflbm_ring* r, const bflbm_params* p);
int bflbm_ring_set_schedule(bflbm_ring* r, int schedule);
int bflbm_ring_init_mixture(bflbm_ring* r);
int bflbm_ring_init_stripe(bflbm_ring* r, double frac);
int bflbm_ring_init_droplet(bflbm_ring* r, double radius);
/* after bflbm_upload_fg on every slab: exchange the uploaded faces, commit, exchange the state faces */
int bflbm_ring_commit_upload(bflbm_ring* r, int reset_step_counter);
int bflbm_ring_set_step_count(bflbm_ring* r, long long steps_done);   /* see bflbm_set_step_count */
/* How the ring moves its faces (the reference's FillBoundary, LBM_binary.H:553-555).  overlap 1 (default): behind the
 * interior sweep, 0: after it (a measurement mode).  transport 0 (default): one gather kernel per face reads the
 * neighbour's planes in place (peer memory over xGMI) where the neighbour is reachable; 1: the copy engine, 38
 * hipMemcpyPeerAsync per face -- no compute units.  bflbm_ring_last_transport: faces the last exchange moved either way. */
int bflbm_ring_set_overlap(bflbm_ring* r, int on);
int bflbm_ring_set_transport(bflbm_ring* r, int transport);
int bflbm_ring_last_transport(const bflbm_ring* r, int* kernel_faces, int* copy_faces);
int bflbm_ring_step(bflbm_ring* r, int nsteps);            /* LBM_timestep x nsteps on the whole lattice */
int bflbm_ring_com_sums(bflbm_ring* r, double sums[4]);    /* update_com sums over all slabs */
int bflbm_ring_mass(bflbm_ring* r, double* rho_sum, double* phi_sum);
int bflbm_ring_sync(bflbm_ring* r);
/* reference-state noise on the ring (see bflbm_set_ref_state); bflbm_ring_prepare_ref hands the global
 * COM of the resident state to the slabs before their noise / hydrovs are read between steps. */
int bflbm_ring_set_ref_state(bflbm_ring* r, const double* rho_eq, const double* phi_eq, const double* rhot_eq, const bflbm_fab* box);
int bflbm_ring_enable_ref_state(bflbm_ring* r, int on, const double com_ref[3]);
int bflbm_ring_prepare_ref(bflbm_ring* r);

/* ---- Replica batch: nreplicas independent periodic lattices of one shape n[3] on one GPU, advanced by one launch per
 * pass (the ensembles of small boxes the reference is run for: several droplets, noise ensembles).
 *  - replica r is an ordinary single-slab lattice (nranks = 1) with its own parameters p[r] (every field may differ,
 *    seed and kBT included), its own state and its own step counter.  One bflbm_batch_step advances every replica by
 *    one LBM_timestep; each replica's result equals, bit for bit, what a lone context with the same parameters, state,
 *    step counter and (forced) exact schedule computes.
 *  - bflbm_batch_replica returns a VIEW: a real bflbm_ctx owned by the batch.  Every per-context call works on it
 *    unchanged (inits, bflbm_upload_fg / bflbm_commit_upload, bflbm_download_fg, bflbm_get_*, bflbm_com_sums,
 *    bflbm_mass, bflbm_set_params / bflbm_get_params, bflbm_step_count / bflbm_set_step_count, the timers, the
 *    structure-factor and droplet calls); its work is enqueued on the batch's stream, so it is ordered against
 *    bflbm_batch_step.  bflbm_set_params on a view takes effect at the next batch step.
 *  - refused on a view (non-zero return, a message naming the batch call to use, state untouched): bflbm_destroy,
 *    bflbm_step / _boundary / _interior / _finish, bflbm_set_schedule, bflbm_set_stream, bflbm_tune_placement,
 *    bflbm_inject_noise, bflbm_set_ref_state / bflbm_enable_ref_state and the halo calls.  Batches do no placement
 *    tuning, take no injected noise and no reference state, and run on one GPU.
 *  - noise: every replica draws its generated noise with its own seed and its own step counter as the noise index, so
 *    bflbm_set_step_count on a view shifts only that replica's stream.  A batch with some replicas at kBT == 0 and
 *    others at kBT != 0 is refused by bflbm_batch_step before any launch (the message names the replicas); different
 *    non-zero kBT within one batch are fine.
 *  - schedules: 0 two-pass, 1 fused (pulled ring), 2 auto (default): 1 at zero noise when the fused workgroups of the
 *    whole batch fill the device's compute units, 0 otherwise (with noise too).  Both are bit-exact, the choice affects
 *    speed only.  Schedule 3 is refused.
 *  - bflbm_batch_create checks its arguments before it touches a device: null pointers, nreplicas < 1 (or > 65535), a
 *    lattice size < 1, a replica too large for the 32-bit offsets of bflbm_create. */
typedef struct bflbm_batch bflbm_batch;
int bflbm_batch_create(const bflbm_params* p /* nreplicas entries */, int nreplicas, const int n[3], int device, bflbm_batch** out);
int bflbm_batch_destroy(bflbm_batch* b);
int bflbm_batch_size(const bflbm_batch* b, int* nreplicas);
int bflbm_batch_replica(bflbm_batch* b, int r, bflbm_ctx** ctx);   /* a view; owned by the batch */
int bflbm_batch_set_schedule(bflbm_batch* b, int schedule);         /* 0, 1 or 2 (auto); 3 is refused */
int bflbm_batch_resolved_schedule(const bflbm_batch* b, int* schedule);
int bflbm_batch_step(bflbm_batch* b, int nsteps);
int bflbm_batch_sync(bflbm_batch* b);

/* The launch plan of the one-pass schedule (1) for a periodic lattice n[3]: the tile shape, the z-chunking and the work
 * list that bflbm_step (nreplicas == 1) or bflbm_batch_step (nreplicas > 1: a batch, with its 256-thread tile when
 * noise != 0) would use, worked out by the planner the launches themselves call.  Host arithmetic only: it needs no
 * device and no context, so a test can state which plan its case exercises.  compute_units > 0 replaces the device's
 * compute-unit count for this call only; 0 is the count the library currently holds (the device's once a context was
 * created on it, 256 before).  out[0..13], the rest zero:
 *    0 tile width, 1 tile height (threads = width x height);
 *    2 tiles in x, 3 tiles in y, 4 strip width in tiles of the column order;
 *    5 planes per chunk, 6 chunks, 7 planes in the last chunk;
 *    8 workgroups per replica, 9 workgroups over all replicas;
 *   10 rounds = ceil(workgroups / compute units);
 *   11 length of one XCD's part of the work list, 12 grid size launched (8 x that; the excess workgroups leave at once);
 *   13 the compute units used.
 * Fails on a null pointer, a size < 1 or too large for a context, nreplicas outside 1..65535, compute_units < 0. */
int bflbm_fused_plan_query(const int n[3], int nreplicas, int noise, int compute_units, int out[16]);

/* The launch plans of the plane-marching sweeps of ONE step of a lone context: schedule 1 (fused, pulled ring; tiles as in
 * bflbm_fused_plan_query, noise != 0 selects the noise tile) or 3 (hand-over, 64 x 4 tiles; noise does not change its plan).
 * slab_planes == 0: the whole periodic lattice n[3], one sweep.  slab_planes > 0: a slab of that many planes of a ring
 * (nranks > 1): the interior sweep over its planes minus the two boundary pairs, and the boundary-pair launch of
 * bflbm_step_boundary.  Worked out by the planner the launches call; host arithmetic only, compute_units as in
 * bflbm_fused_plan_query.  out[0..15]:
 *    0 tile width, 1 tile height;
 *    2 tiles in x, 3 tiles in y, 4 strip width in tiles of the column order;
 *   the interior sweep (all zero for a slab of 4 planes, which has none):
 *    5 planes per chunk, 6 chunks, 7 planes in the last chunk, 8 planes between the starts of consecutive chunks;
 *    9 workgroups, 10 rounds = ceil(workgroups / compute units);
 *   11 length of one XCD's part of the work list, 12 grid size launched (8 x that; the excess workgroups leave at once);
 *   13 the compute units used;
 *   the boundary pairs of a slab (zero for slab_planes == 0): 14 planes of each of its two chunks, 15 planes between their
 *   starts in the one launch that takes both (0: a slab of 4 planes, two launches of one chunk).
 * Fails on a null pointer, a schedule other than 1 or 3, a size < 1 or too large for a context, slab_planes outside
 * {0, 4..nz-4}, compute_units < 0, and for schedule 3 on a lattice the hand-over kernel does not take. */
int bflbm_sweep_plan_query(const int n[3], int schedule, int noise, int slab_planes, int compute_units, int out[16]);

/* ---- Ensemble traces: droplet moments of every replica recorded on the device, read once at the end (the notebooks
 * observe their ensembles every step: nine 32^3 droplets in Surface_Tension.ipynb, a 64^3 droplet's centre of mass 3201
 * times in Droplet_Fluctuation.ipynb, whose estimator where(rho > 0.06, rho, 0) is threshold = 0.06).
 * A trace is attached to one lone single-slab context or one replica batch.  After every `every`-th step taken through
 * its owner it enqueues, on the owner's stream and without a host synchronisation, a reduction of the resident state of
 * every replica into the next slot of a device buffer of `capacity` samples.
 *  - record: BFLBM_TRACE_NREC = 12 doubles per replica and sample; rho is the f-density of the resident state at the
 *    cell (the double bflbm_get_hydrovsbar component 0 holds), x, y, z are cell indices:
 *      [0..9]  sum over the cells with rho > threshold of rho * {1, x, y, z, xx, xy, xz, yy, yz, zz}
 *              (the order of bflbm_droplet_moments)
 *      [10]    sum of rho over all cells
 *      [11]    number of cells with rho > threshold, as a double
 *    threshold = -INFINITY takes every cell; a NaN threshold is refused.
 *  - order: the sums are added in the order of bflbm_droplet_moments: blocks of 256 consecutive sites of the padded
 *    plane by a binary tree, per plane every thread a 256-strided subsequence of the block sums and the same tree, then
 *    the planes 0 ... nz-1 in sequence.  With threshold = -INFINITY entries 0..9 equal bflbm_droplet_moments[0..9] of the
 *    same state bit for bit, entry 10 equals entry 0 and entry 11 is nx ny nz.  A record does not depend on the number
 *    of replicas, on the schedule, or on whether the lattice is a replica or a lone context.
 *  - sampling rule: the trace counts the steps taken through its owner (bflbm_step and the split-step calls, sampled
 *    inside bflbm_step_finish; bflbm_batch_step, sampled after each step's launches) since its creation or reset, and
 *    samples after a step when that count is a multiple of `every`.  bflbm_trace_sample records the resident state now
 *    (e.g. frame 0) without moving the count; bflbm_trace_reset forgets the samples and restarts the count.  Every sample
 *    is labelled on the host with each replica's step counter, so bflbm_set_step_count on one view shifts only that
 *    replica's labels.  A trace only reads the resident state: it works with every schedule and every kind of noise,
 *    follows bflbm_set_stream and changes nothing its owner computes or keeps.
 *  - capacity: bflbm_step, bflbm_batch_step and bflbm_step_boundary first work out how many samples the call would add;
 *    if they do not fit, the call is refused before any launch ("trace full"), state and step counters untouched.
 *    bflbm_trace_sample on a full trace is refused the same way.
 *  - refused at creation (non-zero return, nothing allocated): null arguments, every < 1, capacity < 1, a NaN threshold,
 *    a context with nranks > 1, a replica view (use bflbm_batch_trace_create), an owner that already has a trace, an
 *    open step.  An open step also refuses bflbm_trace_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_trace_read, _count and
 *    _destroy still work, bflbm_trace_sample fails.
 *  - bflbm_trace_read synchronises the owner's stream; no other call of this group does.
 *  - a ring of z-slabs (bflbm_ring_trace_create; the process-per-GPU slabs have no trace): one replica, at most one trace
 *    per ring, labelled with the ring's step counter (slab 0's), sampled by bflbm_ring_step only.  Stage 1 runs on every
 *    slab's own stream over the slab's own planes, z the global plane index, into block sums on the slab's device; slab 0
 *    collects them in global plane order with one contiguous (peer) copy per slab, ordered by events and without a host
 *    synchronisation, and adds them as above on its own stream.  The summation order is therefore exactly a lone
 *    context's: with the bit-exact schedules the record equals the lone lattice's bit for bit, and with threshold =
 *    -INFINITY entries 0..9 equal bflbm_ring_droplet_moments[0..9].  The records live on slab 0's device and
 *    bflbm_trace_read synchronises slab 0's stream alone.  Creation, _sample, _reset and _read are refused while any
 *    slab has an open step.  A ring of one slab gets the lone trace of its only context. */
typedef struct bflbm_trace bflbm_trace;
#define BFLBM_TRACE_NREC 12
int bflbm_trace_create(bflbm_ctx* c, int every, long long capacity, double threshold, bflbm_trace** out);
int bflbm_batch_trace_create(bflbm_batch* b, int every, long long capacity, double threshold, bflbm_trace** out);
int bflbm_ring_trace_create(bflbm_ring* r, int every, long long capacity, double threshold, bflbm_trace** out);
int bflbm_trace_destroy(bflbm_trace* t);
int bflbm_trace_sample(bflbm_trace* t);                 /* record the resident state now (e.g. frame 0) */
int bflbm_trace_reset(bflbm_trace* t);                  /* forget the samples, restart the every-counter */
int bflbm_trace_count(const bflbm_trace* t, long long* nsamples, int* nreplicas);
int bflbm_trace_read(bflbm_trace* t, long long first, long long count,
                     double* rec   /* [count][nreplicas][12] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Interface traces: the height of a density contour above every column of every replica, recorded on the device
 * and read once at the end (the flat-interface height field of Flat_Interface.ipynb, cells 4 and 7-9, whose spectrum
 * <|h_q|^2> is compared with kBT / (gamma q^2); the reference's flat-interface box is 8 x 256 x 64).
 * An interface trace is attached to one lone single-slab context or one replica batch, like an ensemble trace.
 *  - definition (stated here and nowhere else).  Three settings: a field (0 = rho, the density of fluid f; 1 = phi, the
 *    density of fluid g), a `level`, and a z-window [z_lo, z_hi) with 0 <= z_lo, z_hi <= nz and z_hi - z_lo >= 2.
 *    d(z) is the field's density of the resident state at (x, y, z), the sum of the 19 pulled populations in index order:
 *    the double bflbm_get_hydrovsbar component 0 (rho) or 1 (phi) holds.  For every column (x, y) two heights are
 *    recorded, both from scanning z = z_lo+1 ... z_hi-1 upward without a periodic wrap:
 *      rising:   the first z with d(z-1) <  level <= d(z)
 *      falling:  the first z with d(z-1) >= level >  d(z)
 *    and in both cases h = (double)(z-1) + (level - d(z-1)) / (d(z) - d(z-1)): two IEEE subtractions, one division, one
 *    addition, no contraction (linear interpolation, as skimage.find_contours does).  A column without such a pair
 *    records a quiet NaN; a NaN density satisfies neither condition.
 *  - sample: [replica][2][ny][nx] doubles, dense, direction 0 rising, direction 1 falling.
 *  - kernels: stage 1 gives every column a thread, splits the pairs (z-1, z) of the window into contiguous segments and
 *    writes per segment the first rising and first falling candidate (152 B read per site of the window, nothing
 *    written per site); stage 2 takes, per column and direction, the first non-NaN candidate in segment order.  The
 *    number of segments is the library's choice (enough workgroups to fill the device, each segment at least 4 pairs,
 *    an unmeasured heuristic) and changes no bit of a sample; bflbm_iface_geometry reports it.  Both launches go to the
 *    owner's stream; only rho / phi populations are read, nothing of the owner is written.
 *  - sampling rule, capacity, step labels: those of the ensemble traces above.  The trace counts the steps taken through
 *    its owner since its creation or reset and samples after a step when that count is a multiple of `every`;
 *    bflbm_iface_sample records the resident state now without moving the count; bflbm_iface_reset forgets the samples
 *    and restarts the count; every sample is labelled on the host with each replica's step counter.  bflbm_step,
 *    bflbm_batch_step and bflbm_step_boundary refuse, before any launch and with state and counters untouched, a call
 *    whose samples would not fit ("interface trace full"); bflbm_iface_sample on a full trace is refused the same way.
 *  - an owner may carry several interface traces (rho and phi, two levels ...).  After a step the recorders of all kinds
 *    on one owner (ensemble trace, interface traces, a batch's structure-factor accumulators) are served in the order of
 *    their creation; no recorded value depends on that order, and the capacity check covers all of them before the first
 *    launch.
 *  - refused at creation (non-zero return, a message naming the call, nothing allocated): null arguments, a field other
 *    than 0 or 1, a NaN level, a window outside the lattice or shorter than two planes, every < 1, capacity < 1, a
 *    capacity beyond 1 TB of heights, a replica view (use bflbm_batch_iface_create), a context with nranks > 1, an open
 *    step.  An open step also refuses bflbm_iface_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_iface_read, _count,
 *    _geometry and _destroy still work, bflbm_iface_sample fails.
 *  - bflbm_iface_read synchronises the owner's stream; no other call of this group does. */
typedef struct bflbm_iface bflbm_iface;
int bflbm_iface_create(bflbm_ctx* c, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out);
int bflbm_batch_iface_create(bflbm_batch* b, int field, double level, int z_lo, int z_hi, int every, long long capacity, bflbm_iface** out);
int bflbm_iface_destroy(bflbm_iface* t);
int bflbm_iface_sample(bflbm_iface* t);                 /* record the resident state now (e.g. frame 0) */
int bflbm_iface_reset(bflbm_iface* t);                  /* forget the samples, restart the every-counter */
int bflbm_iface_count(const bflbm_iface* t, long long* nsamples, int* nreplicas);
int bflbm_iface_geometry(const bflbm_iface* t, int* nx, int* ny, int* nsegments /* of stage 1 */,
                         int* segment_pairs /* pairs (z-1, z) per segment; the last segment may hold fewer */);
int bflbm_iface_read(bflbm_iface* t, long long first, long long count,
                     double* h     /* [count][nreplicas][2][ny][nx] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Shape traces: the radius of a droplet's density contour along fixed rays from its centre, for every replica,
 * recorded on the device and read once at the end (the droplet shape modes of Droplet_Fluctuation.ipynb, cells 32, 38
 * and 41: the notebook extracts the rho = (max + min) / 2 surface of 2301 frames of a 32^3 droplet with marching cubes,
 * expands its radius r(theta, phi) about the centre of mass in spherical harmonics and follows zeta_1m(t), zeta_2m(t);
 * <|a_lm|^2> = kBT / (gamma (l-1)(l+2)) is the spherical twin of the capillary spectrum of the interface traces).
 * A shape trace is attached to one lone single-slab context or one replica batch, like an interface trace: it is that
 * trace turned from columns into rays.  The projection of the radii onto spherical harmonics is left to the host.
 *  - definition (stated here and nowhere else).  Every operation is an IEEE double operation in the stated order, no
 *    contraction.  Settings: a field (0 = rho, 1 = phi), a `level`, a direction (0 = falling outward, 1 = rising
 *    outward), ndir unit vectors u_j given by the caller as dirs[ndir][3] (the library computes no angles and no
 *    transcendentals), a step delta > 0, a number of steps K >= 1, and either a fixed centre c[3] in cell-index
 *    coordinates (one for all replicas) or, with a null centre, a threshold.
 *      centre (null centre): per replica and sample c_a = m_a / m_0, a = x, y, z, where m are the moments an ensemble
 *        trace with that threshold records (records 1-3 and 0), computed by the same kernels in the same order: the
 *        centre equals records 1-3 / record 0 of bflbm_trace_read of the same state bit for bit.  If no cell is above
 *        the threshold the centre is 0 / 0 = NaN, and so is every radius of that replica.
 *      density at a point p: i_a = floor(p_a), f_a = p_a - (double)i_a; the corner indices i_a and i_a + 1 are wrapped
 *        periodically into [0, n_a), negative i_a included; d_xyz is the field's density of the resident state at the
 *        eight corners (x, y, z each 0 for i_a, 1 for i_a + 1), the double bflbm_get_hydrovsbar component 0 / 1 holds;
 *          c00 = d000 + fx (d100 - d000), c10 = d010 + fx (d110 - d010), c01 = d001 + fx (d101 - d001),
 *          c11 = d011 + fx (d111 - d011);  c0 = c00 + fy (c10 - c00), c1 = c01 + fy (c11 - c01);  d = c0 + fz (c1 - c0).
 *        A point with a coordinate that is NaN or not below 2^30 in magnitude has the density NaN; no index is formed
 *        from it.
 *      ray j: the sample points are p_a = c_a + t_k u_ja with t_k = (double)k delta, k = 0 ... K, and d_k their densities.
 *        falling: the first k >= 1 with d_{k-1} >= level >  d_k gives r_j = delta ((double)(k-1) + (d_{k-1} - level) / (d_{k-1} - d_k))
 *        rising:  the first k >= 1 with d_{k-1} <  level <= d_k gives r_j = delta ((double)(k-1) + (level - d_{k-1}) / (d_k - d_{k-1}))
 *        No such k gives a quiet NaN; a NaN density satisfies neither condition.
 *  - sample: [replica][3 + ndir] doubles: the centre used, then the radii r_0 ... r_{ndir-1}.
 *  - kernels: with a null centre the two kernels of the ensemble trace reduce the moments into a buffer of the shape
 *    trace's own; one kernel writes the chosen field's density of every site of every replica into the shape trace's own
 *    copy (152 B read and 8 B written per site), so that a sample point reads 8 doubles; the ray kernel gives every ray a
 *    lane, splits the pairs (k-1, k) into contiguous segments and writes per segment the first candidate; the last kernel
 *    takes, per ray, the first non-NaN candidate in segment order.  The number of segments is the library's choice
 *    (enough one-wave workgroups for one wave per SIMD, each segment at least 4 pairs, an unmeasured heuristic) and
 *    changes no bit of a sample; bflbm_shape_geometry reports it.  All launches go to the owner's stream, there are no
 *    atomics and no host round trip; nothing of the owner is written (not rho, phi or their validity).
 *  - sampling rule, capacity ("shape trace full", refused before any launch), step labels, detaching, service in
 *    creation order: those of the interface traces above.  An owner may carry several shape traces.
 *  - refused at creation (non-zero return, a message naming the call, nothing allocated): null arguments, a field or a
 *    direction other than 0 or 1, a NaN level, a NaN threshold with a null centre, a non-finite fixed centre, ndir < 1
 *    or > 65536, a direction with a non-finite component or with |u.u - 1| > 1e-6, a step that is not finite or <= 0,
 *    nsteps < 1, every < 1, capacity < 1, a capacity beyond 1 TB of records, a replica view (use
 *    bflbm_batch_shape_create), a context with nranks > 1, an open step.  An open step also refuses bflbm_shape_sample,
 *    _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_shape_read, _count,
 *    _geometry and _destroy still work, bflbm_shape_sample fails.
 *  - bflbm_shape_read synchronises the owner's stream; no other call of this group does.
 *  - out of scope: rings of z-slabs (droplet ensembles are small boxes), and a droplet that diffuses across the periodic
 *    boundary: the centre is the ensemble trace's, which does not unwrap (the rays themselves wrap). */
typedef struct bflbm_shape bflbm_shape;
int bflbm_shape_create(bflbm_ctx* c, int field, double level, int direction, const double* centre_or_null /* [3] */, double threshold,
                       int ndir, const double* dirs /* [ndir][3] */, double step, int nsteps, int every, long long capacity, bflbm_shape** out);
int bflbm_batch_shape_create(bflbm_batch* b, int field, double level, int direction, const double* centre_or_null /* [3] */, double threshold,
                             int ndir, const double* dirs /* [ndir][3] */, double step, int nsteps, int every, long long capacity, bflbm_shape** out);
int bflbm_shape_destroy(bflbm_shape* t);
int bflbm_shape_sample(bflbm_shape* t);                 /* record the resident state now (e.g. frame 0) */
int bflbm_shape_reset(bflbm_shape* t);                  /* forget the samples, restart the every-counter */
int bflbm_shape_count(const bflbm_shape* t, long long* nsamples, int* nreplicas);
int bflbm_shape_geometry(const bflbm_shape* t, int* ndir, int* nsteps, int* nsegments /* of the ray kernel */,
                         int* segment_len /* pairs (k-1, k) per segment; the last segment may hold fewer */);
int bflbm_shape_read(bflbm_shape* t, long long first, long long count,
                     double* r     /* [count][nreplicas][3 + ndir] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Ensemble structure factors: S(k) of every replica of a batch in one batched pass (the reference's live job
 * accumulates structure factors every out_SF_step steps, main_run_job.cpp:299-310, :342-349; Mixture.ipynb reads them).
 * One accumulator serves the whole batch.  A frame enqueues, on the batch's stream and without a host synchronisation,
 * one observation launch over all replicas (only the variables that occur in a pair, densely), one batched hipFFT D2Z
 * (hipfftPlanMany, batch = B x distinct variables) and one accumulation launch; with one bflbm_sf per replica view the
 * same frame is B observation launches, B x distinct variables transforms and B accumulation launches.
 *  - pairs, scale, what, zero_avg, normalisation and output layout (dst[npairs][nz][ny][nx], k = 0 at cell n/2) are
 *    those of bflbm_sf_*.  lb_hydrovars (0: var_a / var_b index hydrovs, != 0: hydrovsbar) is fixed at creation.
 *  - spectra: the accumulator keeps one running sum per replica.  bflbm_batch_sf_get with replica r in 0..B-1 returns
 *    that replica's mean over the frames; replica -1 returns the ensemble mean: per (pair, k) the B per-replica sums
 *    are added in the replica order 0 ... B-1 and multiplied by 1 / (B nsamples), so the result does not depend on launch
 *    geometry.  what = 0 of the ensemble is the magnitude of that complex mean, not a mean of magnitudes.
 *  - sampling rule: every = 0: frames are taken only by bflbm_batch_sf_accumulate.  every >= 1: the accumulator is
 *    attached; it counts the steps taken through bflbm_batch_step since its creation or reset and bflbm_batch_step enqueues
 *    a frame after each step at which that count is a multiple of `every` (the trace's rule; recorders are served in creation order).
 *    bflbm_batch_sf_accumulate is allowed on an attached accumulator and does not move the count, with reset != 0 too
 *    (FortStructure's reset: the running sums and nsamples start again with this frame).  bflbm_batch_sf_reset zeroes the
 *    sums, sets nsamples = 0 and restarts the count.  nsamples counts the frames whose launches were all accepted.
 *  - what is touched on the replicas: the dense fields, the spectra, the running sums and the download buffer belong to
 *    the accumulator; no replica's state or scratch buffer is written.  Only when hydrovs is observed and some replica's
 *    rho / phi arrays are not the densities of its resident state, one density launch over the batch rewrites them for
 *    every replica (a valid replica gets the same doubles again) and marks them valid, as the per-context observables
 *    do.  hydrovsbar needs no densities.  A frame changes nothing the batch computes.
 *  - a batch may hold several accumulators (e.g. one on hydrovs, one on hydrovsbar).
 *  - lifetime: destroying the batch first detaches its accumulators (what is enqueued completes); after that
 *    bflbm_batch_sf_get, _nsamples, _reset and _destroy still work and bflbm_batch_sf_accumulate fails.
 *  - refused (non-zero return, a message naming the call, before any device is touched, nothing allocated): null
 *    arguments, npairs outside 1..32, a variable index outside hydrovs (with lb_hydrovars: outside hydrovsbar),
 *    every < 0; in bflbm_batch_sf_get a replica outside -1..B-1 or what outside 0..2.  A failed allocation or plan
 *    frees what was allocated and reports the sizes; a failed launch reports the HIP error.
 *  - bflbm_batch_sf_get, the two getters below and bflbm_batch_sf_destroy synchronise the batch's stream; no other call
 *    of this group does.
 * bflbm_batch_get_hydrovs / _hydrovsbar: the first ncomp components (1..22, 1..9) of every replica, dst[B][ncomp][nz][ny][nx],
 * with one observation launch, one copy and one synchronisation; the doubles of bflbm_get_hydrovs / _hydrovsbar on the
 * views.  They use a dense buffer owned by the batch, allocated at first use. */
typedef struct bflbm_batch_sf bflbm_batch_sf;
int bflbm_batch_sf_create(bflbm_batch* b, int npairs, const int* var_a, const int* var_b, const double* scale,
                          int lb_hydrovars, int every, bflbm_batch_sf** out);
int bflbm_batch_sf_destroy(bflbm_batch_sf* s);
int bflbm_batch_sf_reset(bflbm_batch_sf* s);                 /* zero the accumulators, nsamples = 0, restart the every-count */
int bflbm_batch_sf_accumulate(bflbm_batch_sf* s, int reset); /* FortStructure(fields, reset) on the resident state of every replica, now */
int bflbm_batch_sf_nsamples(const bflbm_batch_sf* s, long long* n);
int bflbm_batch_sf_get(bflbm_batch_sf* s, int replica, int what, int zero_avg, double* dst);  /* replica -1: ensemble mean */
int bflbm_batch_get_hydrovs(bflbm_batch* b, double* dst, int ncomp);     /* dst[B][ncomp][nz][ny][nx] */
int bflbm_batch_get_hydrovsbar(bflbm_batch* b, double* dst, int ncomp);

/* ---- Spectrum traces: the structure factor of every sample, binned, recorded on the device as a time series and read
 * once at the end (the observable of a coarsening mixture: the shell-averaged S(k, t) of rho - phi and its first moment,
 * the domain length; Mixture.ipynb cell 2 reads the spectra reduced to the kx axis).  The accumulators above keep one
 * running mean of the full 3-D spectrum; a spectrum trace keeps, per sample, replica and pair, one sum per bin.
 * A spectrum trace is attached to one lone single-slab context or one replica batch, like an ensemble trace.
 *  - definition (stated here and nowhere else).  For a pair (a, b) of real fields on the nx x ny x nz periodic lattice,
 *    N = nx ny nz, a^ the unnormalised DFT as in bflbm_sf_*:
 *      S_ab(k) = scale Re(a^(k) conj(b^(k))) / N        over the FULL spectrum,
 *    with the signed integer frequencies kx in (-nx/2, nx/2], ky, kz likewise; only |kx|, |ky|, |kz| enter a bin.  The
 *    imaginary parts of k and -k cancel in every bin, so only the real part is recorded.  A sample holds
 *      sum[bin] = sum over the modes k with bin(k) = bin of S_ab(k).
 *    Bin rules (`kind`):
 *      0, shells:  L = lcm(nx, ny, nz), W = L / max(nx, ny, nz), K2 = (kx L/nx)^2 + (ky L/ny)^2 + (kz L/nz)^2 (an exact
 *                  64-bit integer); bin(k) is the integer s >= 0 with (2s-1)^2 W^2 <= 4 K2 < (2s+1)^2 W^2 (s = 0: the
 *                  upper bound alone, i.e. (2s-1) W <= 2 sqrt(K2) < (2s+1) W): |q| rounded half up in units of the
 *                  smallest non-zero wavenumber of the longest axis, decided in integers, never through a
 *                  floating-point square root.  A cubic box gives the usual round(|k|) shells (16^3: 15 bins
 *                  with 1, 18, 62, 98, 210, 350, ... modes).  Refused where 12 (L/2)^2 does not fit in 63 bits.
 *      1, 2, 3:    axis x, y, z: bin(k) = |kx| (|ky|, |kz|), summed over the other two axes.
 *    zero_avg != 0 (WritePlotFile's flag) leaves the k = 0 mode out of the sum AND out of the count of bin 0.
 *    The number of bins is the largest bin of any mode plus one.  Per bin the geometry fixes
 *      count[bin]: the number of full-spectrum modes in the bin (they add up to N, or N - 1 with zero_avg),
 *      q[bin]:     kind 0: the mean over the bin's modes of |q| = 2 pi sqrt((kx/nx)^2 + (ky/ny)^2 + (kz/nz)^2), a quiet
 *                  NaN for a bin without modes; kinds 1-3: 2 pi bin / n_axis.
 *    From the half spectrum hipFFT returns (mx = 0 ... nx/2) a mode has weight 1 where mx = 0 or 2 mx = nx and weight 2
 *    otherwise; its partner -k lies in the same bin by construction.
 *  - sample: [replica][pair][bin] doubles.  Pairs, scale and lb_hydrovars (0: var_a / var_b index hydrovs, != 0:
 *    hydrovsbar) are those of bflbm_batch_sf_create, fixed at creation.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation (a
 *    batch: one launch over all replicas, only the variables that occur in a pair, into a buffer of the trace; a lone
 *    context: into its scratch state buffer, as bflbm_sf_accumulate), hipFFT D2Z (a batch: one plan of B x distinct
 *    variables transforms; a lone context: one execution per distinct variable), and two binning launches.  At creation
 *    the trace sorts the half-spectrum indices by (bin, index) into a list of 32-bit indices (4 B per half-spectrum
 *    point; refused beyond 2^32 points) and cuts it into chunks of at most 2048 entries that never cross a bin (an
 *    untimed heuristic; bflbm_spectrum_geometry reports the outcome).  Stage 1 gives every (chunk, pair, replica) a
 *    workgroup of 256 threads; a thread adds weight (scale a^) . b^ / N of the chunk's entries tid, tid + 256, ... in
 *    that order, the workgroup adds the 256 sums by a binary tree.  Stage 2 adds, per (bin, pair, replica), the bin's
 *    chunk sums in chunk order and writes the sample's slot.  No atomics: a record depends on the spectra and the
 *    chunk table alone, not on the number of replicas, `every`, the capacity or what else is attached.
 *  - what is touched on the owner: what the accumulators touch.  Observing hydrovs rewrites rho / phi by the density
 *    pass where they are stale; a lone context's scratch state buffer is overwritten (between steps it holds nothing
 *    the next step reads).  The resident state, the step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the ensemble and interface
 *    traces above ("spectrum trace full").  An owner may carry any number of spectrum traces.
 *  - refused at creation (non-zero return, a message naming the call, nothing allocated): null arguments, npairs outside
 *    1..32, a variable outside hydrovs (with lb_hydrovars: outside hydrovsbar), kind outside 0..3, every < 1,
 *    capacity < 1, a capacity beyond 1 TB of sums, the 2^32 and 63-bit limits above, a replica view (use
 *    bflbm_batch_spectrum_create), a context with nranks > 1, an open step, a failed allocation (the message gives the
 *    bytes of each buffer).  An open step also refuses bflbm_spectrum_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_spectrum_read, _count,
 *    _geometry, _bins and _destroy still work, bflbm_spectrum_sample fails.
 *  - creation uploads the tables with blocking copies.  After it only bflbm_spectrum_read and bflbm_spectrum_destroy
 *    synchronise the owner's stream.
 *  - a ring of z-slabs (bflbm_ring_spectrum_create): the same definition, bins, count, q and sample layout with one
 *    replica, labelled with slab 0's step counter, sampled by bflbm_ring_step only; refused like the lone call, and
 *    where ny < nslabs or any slab has an open step.  Slab d of n owns the rows ky in [ny d / n, ny (d+1) / n).  A sample
 *    runs on the slabs' streams, ordered by events and without a host synchronisation (hydrovs under reference-state
 *    noise excepted: the global centre of mass is summed on the host first, as in bflbm_ring_sf_accumulate): every slab
 *    observes its planes into its scratch state buffer and transforms them in (x, y); every slab gathers its rows of
 *    every plane of every slab (a kernel that reads the other slabs' memory in place where it is on the same device or
 *    peer-mapped, strided copies otherwise or with BFLBM_RING_COPY_FALLBACK=1: the same doubles), transforms them along
 *    z and bins them as above over its OWN sorted list (local index (kz nky + ky - ky0) (nx/2+1) + kx, sorted by (bin,
 *    local index), chunks of at most 2048 entries that never cross a bin, k = 0 left out on the slab that holds ky = 0
 *    under zero_avg); slab 0 collects the n arrays of per-slab sums and adds them per (pair, bin) in the order
 *    0 ... n-1 into the slot.  No atomics: a record depends on the spectra, the slabs' tables and the slab count alone.
 *    It differs from a lone lattice's record of the same state by rounding (another FFT, another order).
 *    bflbm_spectrum_geometry reports the chunks summed over the slabs and the most chunks any (slab, bin) has.  The
 *    records live on slab 0's device; bflbm_spectrum_read synchronises slab 0's stream alone, _destroy every slab's.
 *    A ring of one slab gets the lone trace of its only context. */
typedef struct bflbm_spectrum bflbm_spectrum;
int bflbm_spectrum_create(bflbm_ctx* c, int npairs, const int* var_a, const int* var_b, const double* scale /* or NULL */,
                          int lb_hydrovars, int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out);
int bflbm_batch_spectrum_create(bflbm_batch* b, int npairs, const int* var_a, const int* var_b, const double* scale /* or NULL */,
                                int lb_hydrovars, int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out);
int bflbm_ring_spectrum_create(bflbm_ring* r, int npairs, const int* var_a, const int* var_b, const double* scale /* or NULL */,
                               int lb_hydrovars, int kind, int zero_avg, int every, long long capacity, bflbm_spectrum** out);
int bflbm_spectrum_destroy(bflbm_spectrum* t);
int bflbm_spectrum_sample(bflbm_spectrum* t);              /* record the resident state now (e.g. frame 0) */
int bflbm_spectrum_reset(bflbm_spectrum* t);               /* forget the samples, restart the every-counter */
int bflbm_spectrum_count(const bflbm_spectrum* t, long long* nsamples, int* nreplicas);
int bflbm_spectrum_geometry(const bflbm_spectrum* t, int* nbins, int* npairs, long long* nchunks /* of stage 1 */,
                            int* max_chunks_per_bin);
int bflbm_spectrum_bins(const bflbm_spectrum* t, long long* count /* [nbins] */, double* q /* [nbins] */);
int bflbm_spectrum_read(bflbm_spectrum* t, long long first, long long count,
                        double* sums  /* [count][nreplicas][npairs][nbins] */,
                        long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Mode traces: the complex Fourier amplitudes of chosen hydrodynamic variables at chosen wavevectors, recorded on the
 * device as a time series and read once at the end.  The spectrum traces above keep Re(a^ conj(b^)) summed over bins,
 * which drops the phase and mixes the wavevectors; time correlations (the intermediate scattering function
 * <a^(k, t+s) conj(a^(k, t))>, the dynamic structure factor, the decay rates that give viscosity, sound attenuation and
 * diffusion, the Onsager-regression check; Correlation.ipynb) need a^(k, t) of single wavevectors at consecutive steps.
 * A mode trace is attached to one lone single-slab context or one replica batch, like a spectrum trace.
 *  - definition (stated here and nowhere else).  For a real field a on the periodic nx x ny x nz lattice and an integer
 *    wavevector m = (mx, my, mz), any integers, reduced mod n per axis:
 *      a^(m) = sum over (x, y, z) of a(x, y, z) E(m; x, y, z),   E = e^{-2 pi i (mx x / nx + my y / ny + mz z / nz)},
 *    the unnormalised DFT of bflbm_sf_* with numpy's fftn sign: a^(m) == fftn(a)[mz % nz, my % ny, mx % nx] up to rounding.
 *    The phases come from one table per axis, T_n[j] = (cos(2 pi j / n), -sin(2 pi j / n)), j = 0 .. n-1, built once on
 *    the host at creation and exposed by bflbm_modes_phases (host only, needs no device).  The angle is reduced to an
 *    octant in integers: entries with 4 j % n == 0 are exactly (+-1, +-0) or (+-0, +-1), every entry is within 2^-52 of
 *    the real value, and T_n[n - j] == conj(T_n[j]) exactly (the device keeps T_nx and T_ny as their lower halves).
 *    The term of a site is a * ((T_nx[jx] * T_ny[jy]) * T_nz[jz]) with jx = ((mx mod nx) x) mod nx, jy and jz likewise,
 *    every complex product written re = ar br - ai bi, im = ar bi + ai br and left unfused (-ffp-contract=off).  The
 *    factor T_nz[jz] is applied to a plane's sum, not per site: a site adds a * (T_nx[jx] * T_ny[jy]), real times complex.
 *  - order of the sums, fixed by the box, the wavevector list and the variable list alone.  A dense plane z (sites
 *    s = y nx + x) is cut into tiles of 2048 consecutive sites, the last one short (bflbm_modes_geometry reports both
 *    numbers).  Per (replica, z, tile, variable, wavevector): thread t of 256 starts from 0 and adds the terms of the
 *    tile's sites t, t + 256, ..., t + 1792 in that order (a site past the plane adds 0); the 256 sums are added by
 *    the binary tree v[t] += v[t + w], w = 128, 64, ..., 1.  Then per (replica, variable, wavevector): the tiles of a
 *    plane are added in tile order starting from 0, the plane's sum is multiplied by T_nz[jz], and the planes are added
 *    in the sequence z = 0 .. nz-1 starting from 0, as the last step.  No atomics.  A record does not depend on the
 *    number of replicas, `every`, the capacity, the schedule, what else is attached, or lone context versus replica.
 *  - sample: [replica][var][mode][2] doubles (re, im).  `vars` index hydrovs; with lb_hydrovars != 0 they index
 *    hydrovsbar (the spectrum trace's convention).  1..8 distinct variables, 1..64 wavevectors, fixed at creation.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation, as
 *    the spectrum trace's first step (a batch: one launch over all replicas, only the chosen variables, into a buffer of
 *    the trace; a lone context: into its scratch state buffer), the projection kernel (grid tiles x nz x replicas; a
 *    site's values are loaded once, the x and y tables sit in LDS) and the finishing launch (grid (var, mode) x
 *    replicas, the planes spread over the threads first).  Boxes with (nx/2 + 1) + (ny/2 + 1) > 2304 are refused: their
 *    tables do not fit the projection kernel's LDS (36864 + 3072 nvars bytes, 61440 with 8 variables: 2304 table
 *    entries and the tree's two exchange buffers of 2 nvars x 128 and 2 nvars x 64 doubles; the kernel is compiled once
 *    per number of variables;
 *    the finishing kernel uses 4096).  The tile size, the one-wavevector groups and the split of the finish are untimed
 *    heuristics.
 *  - what is touched on the owner: what the spectrum trace's observation touches.  Observing hydrovs rewrites rho / phi
 *    by the density pass where they are stale; a lone context's scratch state buffer is overwritten.  The resident
 *    state, the step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("mode
 *    trace full").  An owner may carry any number of mode traces.
 *  - refused at creation (non-zero return, a message naming the call, nothing allocated): null arguments, counts outside
 *    the limits, a repeated variable, a variable outside its set, every < 1, capacity < 1, a capacity beyond 1 TB of
 *    records, the table limit above, nz > 65535, a replica view (use bflbm_batch_modes_create), a context with
 *    nranks > 1, an open step, a failed allocation (the message gives the bytes of each buffer).  An open step also
 *    refuses bflbm_modes_sample, _reset and _read.  Rings are not served yet; the planes are the last sum so that a ring
 *    of z-slabs can follow.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_modes_read, _count,
 *    _geometry and _destroy still work, bflbm_modes_sample fails.
 *  - creation uploads the tables with blocking copies.  After it only bflbm_modes_read and bflbm_modes_destroy
 *    synchronise the owner's stream. */
typedef struct bflbm_modes bflbm_modes;
int bflbm_modes_create(bflbm_ctx* c, int nvars, const int* vars, int lb_hydrovars, int nmodes, const int* modes /* [nmodes][3] */,
                       int every, long long capacity, bflbm_modes** out);
int bflbm_batch_modes_create(bflbm_batch* b, int nvars, const int* vars, int lb_hydrovars, int nmodes, const int* modes /* [nmodes][3] */,
                             int every, long long capacity, bflbm_modes** out);
int bflbm_modes_destroy(bflbm_modes* t);
int bflbm_modes_sample(bflbm_modes* t);                    /* record the resident state now (e.g. frame 0) */
int bflbm_modes_reset(bflbm_modes* t);                     /* forget the samples, restart the every-counter */
int bflbm_modes_count(const bflbm_modes* t, long long* nsamples, int* nreplicas);
int bflbm_modes_geometry(const bflbm_modes* t, int* nvars, int* nmodes, int* tiles_per_plane, int* tile_sites);
int bflbm_modes_phases(int n, double* table /* [n][2] */); /* T_n; host only */
int bflbm_modes_read(bflbm_modes* t, long long first, long long count,
                     double* amp /* [count][nreplicas][nvars][nmodes][2] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Field statistics: the running mean of chosen fields at every site over the frames taken, and the second moments
 * around it, accumulated on the device (PrintConvergence, Debug.H:275-358 and main_run_job.cpp:422-438, forms the frame
 * mean of rho, phi and rho + phi at every site and writes the equilibrium_* files the reference-state noise consumes;
 * NoiseCovariance.ipynb cell 3 takes the per-site variance of the noise moments over 200 frames).  The mode and spectrum
 * traces give statistics in k-space, the ensemble trace 12 numbers per lattice; this gives <x>(site) and <x y>(site).
 * A field statistic is an accumulator in the sense of the ensemble structure factors: unbounded capacity, every = 0 means
 * fed by bflbm_fstat_sample only.  It is attached to one lone single-slab context, one replica batch or one ring.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components; 2: the noise moments of bflbm_get_noise, 38 components, 0..18 of fluid f, 19..37 of fluid g), nvars in
 *    1..8 distinct component indices of that source, and npairs in 0..16 pairs (a, b) of variable SLOTS (positions in the
 *    variable list), a == b allowed.  For every replica and site, with x_v(t) the value of variable v in frame
 *    t = 0 .. N-1, the frames in recording order:
 *      first[v] = x_v(0)
 *      sum[v]   = ((x_v(0) + x_v(1)) + x_v(2)) + ...                          a plain sequential sum
 *      prod[p]  = sum over t, in order and starting from +0.0, of (x_a(t) - first[a]) * (x_b(t) - first[b])
 *    the product formed first and then added, never contracted (-ffp-contract=off); frame 0 contributes +0.0.
 *    Derived when read, N the number of frames:
 *      mean[v] = sum[v] * (1.0 / N)              the arithmetic of PrintConvergence's mean followed by mult(1./Nsteps)
 *      cov[p]  = prod[p] * (1.0 / N) - (mean[a] - first[a]) * (mean[b] - first[b])
 *    The shift by the first frame is there so that a fluctuation of 1e-3 around a density of 1 does not lose six digits
 *    in the difference of two numbers near 1; it changes no covariance in exact arithmetic.  cov is the covariance with
 *    the divisor N.  The raw second moment about zero is cov + mean[a] mean[b], not prod / N.
 *    Ensemble values of a batch of B replicas (replica = -1): mean is the replicas' sum added in the order 0 ... B-1
 *    starting from 0, times 1.0 / (B N); cov is the replicas' cov, each around its own replica's mean, added in the order
 *    0 ... B-1 starting from 0, times 1.0 / B: the mean WITHIN-replica covariance, not the covariance of the pooled
 *    frames.  sum, first and prod have no ensemble form.
 *    analysis.field_statistics restates all of this in numpy, operation for operation.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation (a
 *    lone context and every slab of a ring: into the scratch state buffer, hydrovs and noise after the density pass and
 *    the reference-state preparation of bflbm_sf_accumulate / bflbm_ring_sf_accumulate, which sums the centre of mass on
 *    the host while reference-state noise is active; a batch: one launch over all replicas, only the chosen variables,
 *    into a buffer of the recorder), then ONE accumulation launch over the dense sites: a thread takes two neighbouring
 *    sites per turn (16-byte accesses where a volume is 16-byte aligned, a scalar tail where the site count is odd),
 *    loads the chosen variables once, updates sum, writes first on frame 0 and updates every prod.  Whether a frame is
 *    frame 0 is decided on the host.  The kernel is compiled once per number of variables; no atomics, no LDS, no
 *    scratch.  Every value depends on the site's own frames alone: not on the launch geometry, the number of replicas,
 *    the slab count, `every` or what else is attached.
 *  - storage: (2 nvars + npairs) x B x n doubles, n the sites, beside one download buffer of n doubles and a batch's dense
 *    fields B x nvars x n.  On a ring every slab keeps the accumulators of its own planes on its own device and feeds
 *    them on its own stream; a sample needs no event between the slabs.  This is the one recorder whose records do not
 *    live on slab 0.
 *  - what is touched on the owner: what the observation touches.  Observing hydrovs rewrites rho / phi by the density
 *    pass where they are stale; a context's scratch state buffer is overwritten (between steps it holds nothing the
 *    next step reads).  The resident state, the step counters and everything the owner computes are unchanged.
 *  - sampling rule: that of the ensemble structure factors.  every >= 1: a frame after each step through the owner
 *    (bflbm_step and the split-step calls, bflbm_batch_step, bflbm_ring_step) at which the count of steps since creation or
 *    reset is a multiple of `every`; recorders are served in creation order.  bflbm_fstat_sample takes a frame of the
 *    resident state now and does not move the count.  bflbm_fstat_reset sets N = 0 and restarts the count: the next frame
 *    is frame 0 again and overwrites every accumulator.  An owner may carry any number of field statistics.
 *  - bflbm_fstat_get(s, what, index, replica, dst): what 0 sum, 1 mean, 2 first, 3 prod, 4 cov; index a variable slot for
 *    0, 1, 2 and a pair index for 3, 4; replica 0 .. B-1, or -1 for the ensemble value (what 1 and 4 only; a lone context and a
 *    ring have B = 1); dst[nz][ny][nx] of the whole
 *    lattice.  One small kernel forms mean, cov and the ensemble values into the download buffer; a ring is gathered slab
 *    by slab.
 *  - refused (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's recorder list
 *    untouched): null arguments, a source outside 0..2, nvars outside 1..8, npairs outside 0..16, a component index
 *    outside the source, a repeated variable, a pair slot outside 0..nvars-1, every < 0, source 2 on a batch (its
 *    observation has no noise form), a replica view (use bflbm_batch_fstat_create), a context with nranks > 1, an open
 *    step, a failed allocation (the message gives the bytes).  In bflbm_fstat_get: what outside 0..4, an index or replica
 *    out of range, replica -1 with what other than 1 and 4, N = 0.  An open step also refuses _sample, _reset and _get.
 *  - lifetime: the recorder owns its buffers.  Destroying the owner first detaches it: bflbm_fstat_get, _count, _reset
 *    and _destroy still work, bflbm_fstat_sample fails.
 *  - only bflbm_fstat_get and bflbm_fstat_destroy synchronise the owner's stream (a ring: every slab's).
 *  - a ring of one slab gets the lone recorder of its only context. */
typedef struct bflbm_fstat bflbm_fstat;
int bflbm_fstat_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a /* or NULL if npairs == 0 */,
                       const int* pair_b, int every, bflbm_fstat** out);
int bflbm_batch_fstat_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                             int every, bflbm_fstat** out);
int bflbm_ring_fstat_create(bflbm_ring* r, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                            int every, bflbm_fstat** out);
int bflbm_fstat_destroy(bflbm_fstat* s);
int bflbm_fstat_sample(bflbm_fstat* s);                    /* take a frame of the resident state now (e.g. frame 0) */
int bflbm_fstat_reset(bflbm_fstat* s);                     /* N = 0, restart the every-count: the next frame is frame 0 */
int bflbm_fstat_count(const bflbm_fstat* s, long long* nsamples, int* nreplicas);
int bflbm_fstat_get(bflbm_fstat* s, int what, int index, int replica, double* dst /* [nz][ny][nx] */);

/* ---- Profile traces: the sums of chosen fields, and of chosen products of them, over every lattice plane normal to one
 * axis, recorded on the device as a time series and read once at the end.  The profile across a flat interface is what
 * the reference's surface-tension work starts from: surface_tension_predict.ipynb (cell 9) averages rho and phi over
 * the planes of a stripe box and compares rho(z) with its interface ODE, and Surface_Tension.ipynb (cell 2) derives the
 * pressure tensor P_ab = [...] delta_ab - 1/2 G cs^4 (d_a rho d_b phi + d_a phi d_b rho), whose normal-minus-tangential
 * part integrates to the surface tension.  hydrovs carries af = -cs2 alpha0 grad phi and ag = -cs2 alpha0 grad rho, so
 * plane sums of af_a ag_a give that integrand with no new stencil (analysis.pressure_profile).  A profile trace is
 * attached to one lone single-slab context, one replica batch or one ring.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), nvars in 1..8 distinct component indices of that source, npairs in 0..16 pairs (a, b) of variable SLOTS
 *    (positions in the variable list), a == b allowed, and an axis (0: x, 1: y, 2: z) of extent n_a.  With
 *    Q = nvars + npairs, entry (q, i) of a sample is the sum, over the sites of the lattice plane with coordinate i along
 *    the axis, of x_q for q < nvars and of x_a * x_b for the pair q - nvars: the product formed first and then added,
 *    never contracted (-ffp-contract=off).  These are sums, not means: the reader divides by the plane's site count,
 *    nx ny nz / n_a.  analysis.plane_profiles restates this in numpy, operation for operation and in the order below.
 *  - order of the sums, fixed by the box and the axis alone.  Every sum starts from +0.0.  Stage 1 works per lattice
 *    plane z, whatever the axis, on the dense plane (sites s = y nx + x):
 *      axis z: the plane is cut into tiles of 2048 consecutive sites, the last one short.  Per (q, tile): thread t of 256
 *        adds the terms of the tile's sites t, t + 256, ..., t + 1792 in that order (a site past the plane adds 0); the
 *        256 sums are added by the binary tree v[t] += v[t + w], w = 128, 64, ..., 1.  One partial per (q, tile).
 *      axis y: per (q, row y of the plane): lane l of 64 adds the terms of x = l, l + 64, ... in that order; the 64 sums
 *        are added by the tree v[l] += v[l + w], w = 32, 16, ..., 1.  One partial per (q, y).
 *      axis x: per (q, column x of the plane): the rows are cut into chunks of 64, the last one short; a chunk's terms are
 *        added sequentially in y, and the chunks' sums are added in chunk order.  One partial per (q, x).
 *    Stage 2: axis z adds the tiles of a plane in tile order; axes x and y add the planes' partials in the sequence
 *    z = 0 .. nz-1, as the last step, so that a ring of z-slabs gives the same record.  No atomics.  A record does not
 *    depend on the number of replicas, `every`, the capacity, the schedule, the slab count, what else is attached, or
 *    lone context versus replica.  bflbm_profile_geometry reports Q, n_a, the sites of a work item (2048 for axis z, the
 *    64 lanes for axis y, the 64 rows of a chunk for axis x) and the partials stage 1 leaves per (q, plane): the tiles
 *    per plane for axis z, n_a for axes x and y.
 *  - sample: [replica][q][n_a] doubles.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation,
 *    exactly as the mode trace takes it (a lone context and every slab of a ring: into the scratch state buffer; a batch:
 *    one launch over all replicas, only the chosen variables, into a buffer of the trace); the plane kernel, grid (work
 *    items of a plane) x planes x replicas, compiled once per number of variables: a site's variables are loaded once,
 *    the products are formed in registers with the slots picked by selects; for axes z and y two neighbouring lanes
 *    fetch two consecutive turns with one 16-byte load each and swap halves where the volume is 16-byte aligned and
 *    both turns lie inside the plane (row), 8-byte loads otherwise and for axis x, where a lane owns a column; the first
 *    two levels of axis z's tree and axis x's chunk sums pass through LDS (1536 (nvars + 16) bytes), the last six
 *    levels and axis y's tree are lane shifts; then the finishing launch, one thread per (q, i), straight into the slot
 *    [sample][replica].  No atomics, no scratch.  The tile, lane and chunk sizes are untimed heuristics.
 *  - a ring of z-slabs: every slab runs stage 1 on its own stream over its own planes into [nzl][Q][W], W the partials
 *    per (q, plane) above; slab 0 takes every other slab's block with one contiguous (peer) copy after that slab's
 *    event, in global plane order, and the unchanged stage 2 runs on slab 0 (the ensemble trace's scheme).  With the
 *    bit-exact schedules the record equals the lone lattice's bit for bit.  A ring of one slab gets the lone recorder of
 *    its only context.  Slabs stepped by hand are not served.
 *  - what is touched on the owner: what the mode trace's observation touches.  Observing hydrovs rewrites rho / phi by
 *    the density pass where they are stale; a context's scratch state buffer is overwritten.  The resident state, the
 *    step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("profile
 *    trace full").  An owner may carry any number of profile traces.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments, a source outside 0..1, an axis outside 0..2, nvars outside 1..8, npairs
 *    outside 0..16, a repeated variable, a component index outside its source, a pair slot outside 0..nvars-1,
 *    every < 1, capacity < 1, a capacity beyond 1 TB of records, nz > 65535, a replica view (use
 *    bflbm_batch_profile_create), a context with nranks > 1, an open step, a failed allocation (the message gives the
 *    bytes of each buffer).  An open step also refuses bflbm_profile_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_profile_read, _count,
 *    _geometry and _destroy still work, bflbm_profile_sample fails.  bflbm_profile_destroy(NULL) returns 0.
 *  - only bflbm_profile_read and bflbm_profile_destroy synchronise the owner's stream (a ring: destroy every slab's). */
typedef struct bflbm_profile bflbm_profile;
int bflbm_profile_create(bflbm_ctx* c, int source, int axis, int nvars, const int* vars, int npairs,
                         const int* pair_a /* or NULL if npairs == 0 */, const int* pair_b, int every, long long capacity, bflbm_profile** out);
int bflbm_batch_profile_create(bflbm_batch* b, int source, int axis, int nvars, const int* vars, int npairs,
                               const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_profile** out);
int bflbm_ring_profile_create(bflbm_ring* r, int source, int axis, int nvars, const int* vars, int npairs,
                              const int* pair_a, const int* pair_b, int every, long long capacity, bflbm_profile** out);
int bflbm_profile_destroy(bflbm_profile* t);
int bflbm_profile_sample(bflbm_profile* t);                /* record the resident state now (e.g. frame 0) */
int bflbm_profile_reset(bflbm_profile* t);                 /* forget the samples, restart the every-counter */
int bflbm_profile_count(const bflbm_profile* t, long long* nsamples, int* nreplicas);
int bflbm_profile_geometry(const bflbm_profile* t, int* nsums /* Q */, int* n_axis, int* tile_sites, int* tiles_per_plane);
int bflbm_profile_read(bflbm_profile* t, long long first, long long count,
                       double* sums /* [count][nreplicas][Q][n_a] */,
                       long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Histogram traces: the counts of the sites of chosen fields over fixed bins, and of chosen pairs of fields over the
 * product of two binnings, recorded on the device as a time series of 64-bit integers and read once at the end.  Every
 * other recorder reduces a sample to sums; this one records a distribution: the single-site velocity PDF against
 * Maxwell-Boltzmann and the PDF of the noise modes themselves, P(rho) and P(phi) turning bimodal while a mixture demixes
 * (Mixture.ipynb, Correlation.ipynb), the occupancy of the (rho, phi) plane, and what the reference's drivers print first
 * (compute_multifab_fluctuation, PrintDensityFluctuation, MultiFabNANCheck, Debug.H:136-228): is the field still finite,
 * and how wide is it.  A histogram trace is attached to one lone single-slab context, one replica batch or one ring.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components; 2: the noise moments of bflbm_get_noise, 38 components, 0..18 of fluid f, 19..37 of fluid g; a lone
 *    context or a ring only), nvars in 1..8 distinct component indices of that source, per variable slot v a range
 *    lo_v < hi_v, both finite, and nbins_v in 1..4096, and npairs in 0..4 pairs (a, b) of variable SLOTS, a != b.
 *    Binning rule for variable v and a site value x, every operation an IEEE double operation:
 *      scale_v = (double)nbins_v / (hi_v - lo_v)        once on the host, one division; must be finite and positive
 *      t = (x - lo_v) * scale_v                          the subtraction first, the multiplication second, never
 *                                                        contracted or reassociated (-ffp-contract=off)
 *      t is NaN: the site goes to the variable's `nan` counter; else t < 0: to `below`; else t >= nbins_v: to `above`;
 *      else to bin (int)t.
 *    So -0.0 lands in bin 0 of a range from 0, +inf in `above`, -inf in `below`, and a value just under hi_v whose t
 *    rounds to nbins_v in `above`: that is the rule, not an error.  A pair uses its two slots' own binnings: the site
 *    goes to cell [ia][ib] when both coordinates are in a bin, and to the pair's single `outside` counter otherwise.
 *    analysis.field_histograms restates this in numpy, operation for operation.
 *  - sample: per replica C 64-bit signed counts: per variable, in slot order, nbins_v bins, then below, above, nan;
 *    then per pair nbins_a x nbins_b cells in row-major order ([ia][ib]), then outside.  C <= 16384.  Every variable
 *    block and every pair block of a sample sums to nx ny nz.  The sums are of integers: a record does not depend on
 *    the number of replicas, `every`, the capacity, the schedule, the slab count, what else is attached, lone context
 *    versus replica, or the launch geometry.
 *  - bflbm_hist_geometry reports C, the number of blocks nvars + npairs, the offset and the length of every block (the
 *    variables first, then the pairs; arrays of nvars + npairs entries, at most 12), the sites of a work item (2048),
 *    the workgroups per replica of the counting launch over the whole box (a slab of a ring launches its own share)
 *    and the 32-bit LDS counters of the instantiation that serves C (4096 for C <= 4096, else 16384).
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation,
 *    exactly as the profile trace takes it (source 2 as the field statistics take it); ONE counting launch, compiled
 *    once per number of variables and per LDS size, grid (workgroups, 1, replicas) of 256 threads: a workgroup keeps all
 *    C counters of its replica as 32-bit words in LDS (16384 bytes for C <= 4096, else 65536 bytes: two workgroups in a
 *    CU's 160 KiB) and strides over the tiles of 2048 consecutive sites of the replica's dense volume; a thread takes
 *    two neighbouring sites per turn, loads their variables once (one 16-byte access per variable where the volume is
 *    16-byte aligned and both sites exist, 8-byte loads otherwise), derives every bin index and every pair cell from
 *    those registers and adds 1 to each counter in LDS (one add per run of equal counters within a wave, the remedy for
 *    a zero-noise mixture whose every lane meets the same counter, was measured and was no faster: DESIGN.md section 8);
 *    at its end the workgroup adds every non-zero counter to the replica's 64-bit totals with one global integer add
 *    each (this form ships; a [workgroups][C] stage buffer was not built).  The workgroups per replica are
 *    min(tiles, max(1, 512 / replicas)), raised where a workgroup would otherwise meet 2^31 sites, so that no 32-bit
 *    counter can wrap before it is flushed.  Then ONE finishing launch writes the totals straight into the slot
 *    [sample][replica][C] and sets them back to zero.  No scratch.
 *  - a ring of z-slabs: every slab counts its own planes on its own stream into its own [C] 64-bit totals and finishes
 *    them into a block of its own; slab 0 takes each block with one (peer) copy after that slab's event and its
 *    finishing launch adds them to its own totals into the slot (the ensemble trace's scheme, events in both directions,
 *    no host synchronisation).  With the bit-exact schedules the record equals the lone lattice's exactly.  A ring of one
 *    slab gets the lone recorder of its only context.  Slabs stepped by hand are not served.
 *  - what is touched on the owner: what the profile trace's observation touches.  Observing hydrovs rewrites rho / phi by
 *    the density pass where they are stale; a context's scratch state buffer is overwritten.  The resident state, the
 *    step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("histogram
 *    trace full").  An owner may carry any number of histogram traces; other bins for a pair: a second trace.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments (the range and bin arrays included), a source outside 0..2, nvars outside
 *    1..8, npairs outside 0..4, a repeated variable, a component index outside its source, a pair slot outside
 *    0..nvars-1, a pair of a slot with itself, a non-finite lo or hi, hi <= lo, a scale that is not finite and positive,
 *    nbins outside 1..4096, C > 16384, every < 1, capacity < 1, a capacity beyond 1 TB of records, source 2 on a batch
 *    (its observation has no noise form), a replica view (use bflbm_batch_hist_create), a context with nranks > 1, an
 *    open step, a failed allocation (the message gives the bytes of each buffer).  An open step also refuses
 *    bflbm_hist_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_hist_read, _count,
 *    _geometry and _destroy still work, bflbm_hist_sample fails.  bflbm_hist_destroy(NULL) returns 0.
 *  - only bflbm_hist_read and bflbm_hist_destroy synchronise the owner's stream (a ring: destroy every slab's). */
typedef struct bflbm_hist bflbm_hist;
int bflbm_hist_create(bflbm_ctx* c, int source, int nvars, const int* vars, const double* lo /* [nvars] */, const double* hi,
                      const int* nbins, int npairs, const int* pair_a /* or NULL if npairs == 0 */, const int* pair_b,
                      int every, long long capacity, bflbm_hist** out);
int bflbm_batch_hist_create(bflbm_batch* b, int source, int nvars, const int* vars, const double* lo, const double* hi,
                            const int* nbins, int npairs, const int* pair_a, const int* pair_b,
                            int every, long long capacity, bflbm_hist** out);
int bflbm_ring_hist_create(bflbm_ring* r, int source, int nvars, const int* vars, const double* lo, const double* hi,
                           const int* nbins, int npairs, const int* pair_a, const int* pair_b,
                           int every, long long capacity, bflbm_hist** out);
int bflbm_hist_destroy(bflbm_hist* t);
int bflbm_hist_sample(bflbm_hist* t);                      /* record the resident state now (e.g. frame 0) */
int bflbm_hist_reset(bflbm_hist* t);                       /* forget the samples, restart the every-counter */
int bflbm_hist_count(const bflbm_hist* t, long long* nsamples, int* nreplicas);
int bflbm_hist_geometry(const bflbm_hist* t, int* ncounters /* C */, int* nblocks, int* offsets /* [nvars + npairs] */,
                        int* lengths /* [nvars + npairs] */, int* tile_sites, int* groups, int* lds_counters);
int bflbm_hist_read(bflbm_hist* t, long long first, long long count,
                    long long* counts /* [count][nreplicas][C] */,
                    long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Morphology traces: the four Minkowski functionals (volume, interface area, mean breadth, Euler characteristic) of
 * a thresholded field, recorded on the device as a time series of 64-bit integer counts and read once at the end.  Every
 * other recorder records a sum, a spectrum, a height, a radius or a distribution; this one records the shape of the
 * domains: the interface area S(t) of a coarsening mixture and with it the real-space domain size L = V_box / S, the Euler
 * characteristic chi(t), strongly negative for a bicontinuous sponge and positive once it has broken into droplets, and
 * the number of droplets, which for simply connected droplets is chi itself (has a satellite pinched off, per replica of
 * a batch).  On a lattice these are sums of integer counts over 2 x 2 x 2 neighbourhoods (Michielsen and De Raedt's
 * counting on the cubical complex).  A morphology trace is attached to one lone single-slab context or one replica batch.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), one component index v of that source, nlevels in 1..8 finite levels t_l and a side.  Side 0 occupies
 *    the site (x, y, z) at level l when v[z][y][x] >= t_l, side 1 when v[z][y][x] < t_l (IEEE double comparisons: a NaN
 *    occupies nothing on either side, -0.0 equals +0.0).  Let o(x, y, z) in {0, 1} be the occupancy at one level and `+`
 *    on a coordinate its periodic successor (n - 1 -> 0; an extent of 1 is its own successor).  Every site adds
 *      N3 += o(x,y,z)
 *      N2 += [o(x,y,z) | o(x+,y,z)] + [o(x,y,z) | o(x,y+,z)] + [o(x,y,z) | o(x,y,z+)]
 *      N1 += [OR of o over the 2 x 2 block (y,y+) x (z,z+) at x] + [the same over (x,x+) x (z,z+) at y]
 *            + [the same over (x,x+) x (y,y+) at z]               the edges along x, y and z
 *      N0 += [OR of o over the 2 x 2 x 2 block (x,x+) x (y,y+) x (z,z+)]
 *    These are the cubes, faces, edges and vertices of the union of the closed unit voxels of the occupied sites on the
 *    3-torus, each element counted once; the rule holds for extents 1 and 2 as it stands.  Closed voxels: the set is
 *    26-connected, its complement 6-connected.  From the counts
 *      V = N3          S = -6 N3 + 2 N2          2B = 3 N3 - 2 N2 + N1          chi = -N3 + N2 - N1 + N0
 *    (volume in cells, area in cell faces, twice the mean breadth in cell edges, the Euler characteristic).  An a x b x c
 *    cuboid gives (abc, 2(ab + bc + ca), a + b + c, 1), the full box (nx ny nz, 0, 0, 0).
 *    analysis.minkowski_counts restates the rule in numpy, analysis.minkowski_functionals the four lines above.
 *  - sample: [replica][nlevels][4] 64-bit signed counts, N3, N2, N1, N0 per level in the order of the levels.  The sums
 *    are of integers: a record does not depend on the number of replicas, `every`, the capacity, the schedule, what else
 *    is attached, lone context versus replica, or the launch geometry.
 *  - bflbm_morph_geometry reports nlevels, the plane sites of a work item's tile (1024), its planes Zc, the work items
 *    per replica (tiles per plane x chunks of Zc planes) and the workgroups of the counting launch over all replicas
 *    (one work item each: the launch does not stride).
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation of
 *    the one variable, exactly as the histogram trace takes it; ONE counting launch, compiled once per number of levels
 *    (the 4 nlevels counters of a wave live in scalar registers, which only static indices reach), grid (work items, 1,
 *    replicas) of 256 threads: a work item is a tile of 1024 consecutive plane sites p = y nx + x times a chunk of Zc
 *    planes; a thread marches four sites along z, per plane loads each site's value and those of its x+, y+ and x+y+
 *    neighbours (cached re-loads; the wraps inside the row and inside the plane are offsets computed once), forms the
 *    8-bit level mask of every value and the OR-masks of the (x,x+), (y,y+) and (x,x+,y,y+) neighbourhoods, keeps those
 *    of the previous plane in one register, so that a cell between the planes z and z+ costs one new plane, and the last
 *    chunk's z+ wraps to plane 0; per level and counter one population count of a wave ballot is added into a
 *    wave-uniform 32-bit counter (integers only, no per-lane counters, no cross-lane reduction); after the march one LDS
 *    add per wave and counter and one global 64-bit integer add per non-zero counter and workgroup into the replica's
 *    totals.  A workgroup meets 1024 Zc <= 65536 cells and a cell adds at most 3 to a counter, so no 32-bit counter can
 *    wrap.  Zc is the largest of 64, 32, 16, 8 that leaves 1024 work items over all replicas, else 8, and at most nz (an
 *    untimed heuristic, like the tile).  Expected memory traffic: 8 (Zc + 1) / Zc bytes per site plus a tile's one-row
 *    halo, 8 nx / 1024 bytes per site.  Then ONE finishing launch, the histogram trace's, writes the totals straight
 *    into the slot [sample][replica][nlevels][4] and sets them back to zero.  No scratch, 128 bytes of static LDS.
 *  - no ring: a cell crosses the slab boundary and needs the next slab's first observed plane, which no slab of a ring
 *    holds.  There is no bflbm_ring_morph_create (the interface trace's exclusion).
 *  - what is touched on the owner: what the histogram trace's observation touches.  Observing hydrovs rewrites rho / phi
 *    by the density pass where they are stale; a context's scratch state buffer is overwritten.  The resident state, the
 *    step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces
 *    ("morphology trace full").  An owner may carry any number of morphology traces: rho and phi, or both sides.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments (before any device is touched), nlevels outside 1..8, a non-finite level, a
 *    side other than 0 or 1, a source outside 0..1, a component index outside its source, every < 1, capacity < 1, a
 *    capacity beyond 1 TB of records, a plane of more than 2^30 sites, a replica view (use bflbm_batch_morph_create), a
 *    context with nranks > 1, an open step, a failed allocation (the message gives the bytes of each buffer).  An open
 *    step also refuses bflbm_morph_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_morph_read, _count,
 *    _geometry and _destroy still work, bflbm_morph_sample fails.  bflbm_morph_destroy(NULL) returns 0.
 *  - only bflbm_morph_read and bflbm_morph_destroy synchronise the owner's stream. */
typedef struct bflbm_morph bflbm_morph;
int bflbm_morph_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels /* [nlevels] */, int side,
                       int every, long long capacity, bflbm_morph** out);
int bflbm_batch_morph_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side,
                             int every, long long capacity, bflbm_morph** out);
int bflbm_morph_destroy(bflbm_morph* t);
int bflbm_morph_sample(bflbm_morph* t);                    /* record the resident state now (e.g. frame 0) */
int bflbm_morph_reset(bflbm_morph* t);                     /* forget the samples, restart the every-counter */
int bflbm_morph_count(const bflbm_morph* t, long long* nsamples, int* nreplicas);
int bflbm_morph_geometry(const bflbm_morph* t, int* nlevels, int* tile_sites, int* chunk_planes /* Zc */,
                         int* items /* work items per replica */, int* groups /* workgroups over all replicas */);
int bflbm_morph_read(bflbm_morph* t, long long first, long long count,
                     long long* counts /* [count][nreplicas][nlevels][4] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Chord traces: the run-length (chord-length) distributions of a thresholded field along x, y and z, recorded on the
 * device as a time series of 64-bit integer counts and read once at the end.  The morphology trace says how much interface
 * there is, the cluster and component traces into how many pieces the set falls; this one records the distribution of the
 * domain widths along a direction, the standard real-space measure of a coarsening or arrested mixture: its mean per axis
 * is the stereological domain size 4V/S, its tail tells a bicontinuous sponge from a droplet phase, and the three axes
 * against each other show anisotropy (a stripe, a sheared or confined mixture, lamellae forming), which the isotropic
 * shell spectrum and the Minkowski counts average away.  A chord trace is attached to one lone single-slab context or one
 * replica batch.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), one component index v of that source, nlevels in 1..8 finite levels t_l, a side, and max_length M in
 *    1..4096.  The occupancy is the morphology trace's: side 0 occupies the site (x, y, z) at level l when
 *    v[z][y][x] >= t_l, side 1 when v[z][y][x] < t_l, a NaN occupies nothing on either side.  For an axis a of x, y, z
 *    with extent n_a the periodic box has nsites / n_a lines, each the n_a sites that differ in the coordinate a only.
 *      - A line whose sites are all occupied is a spanning line and carries no chord (on an axis of extent 1: every
 *        occupied site).
 *      - On every other line each maximal run of consecutive occupied sites is one chord of length l, 1 <= l <= n_a - 1.
 *        The line is periodic: a run that passes from n_a - 1 to 0 is one chord.
 *  - sample: [replica][nlevels][W] 64-bit signed integers, W = 1 + 3 (3 + M), per level in the order of the levels:
 *      word 0                 V, the occupied sites
 *      then one block of 3 + M words per axis, in the order x, y, z:
 *        chords               the chords of the axis
 *        spanning             its spanning lines
 *        long_sites           the sum of l over the chords with l >= M
 *        h[1] .. h[M]         h[l]: the chords of length l for l < M; h[M]: those with l >= M
 *    Identities, exact on every state: per axis sum_l h[l] = chords and
 *    sum_{l<M} l h[l] + long_sites + n_a spanning = V; over the axes chords_x + chords_y + chords_z = N2 - 3 N3 of the
 *    morphology trace's counts at the same level and side, that is S = 2 (chords_x + chords_y + chords_z): every chord has
 *    two ends and every end is one exposed face.  The mean chord along a is (V - n_a spanning) / chords.  The sums are of
 *    integers: a record does not depend on the number of replicas, `every`, the capacity, the schedule, what else is
 *    attached, lone context versus replica, or the launch geometry.  analysis.chord_counts restates the rule in numpy,
 *    analysis.chord_blocks the layout.
 *  - bflbm_chord_geometry reports nlevels, M, W, the 32-bit LDS counters of a workgroup (nlevels W) and the workgroups of
 *    the x, y and z launches over all replicas.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation of
 *    the one variable, exactly as the morphology trace takes it; THREE counting launches, compiled once per number of
 *    levels, 256 threads each, every workgroup with a private copy of its replica's record as nlevels W 32-bit counters
 *    in dynamic LDS (4 nlevels W bytes, at most 64 KiB; no static LDS) and one 64-bit global integer add per non-zero
 *    counter at its end.  The x launch: a wave takes a row 64 sites at a turn, one wave ballot per level gives the
 *    block's occupancy mask, the runs that close inside the block are found from the mask by bit operations at the lane
 *    of the closing zero, the open run is carried to the next block as a wave-uniform length, and the run through site 0
 *    is joined with the run that ends at nx - 1 when the row is finished; V is counted here.  The y and the z launch are
 *    one kernel with the stride and the line map as arguments: a work item is 256 consecutive lines p = o nx + x, the
 *    lanes lie along x so that every load is a coalesced row segment, a lane marches its line and keeps per level the
 *    open run, the head run and a bit "a zero was seen" in registers and joins head and tail at the end.  A line is
 *    handled whole by one wave (x) or one lane (y, z): no chunks, no merge pass, no grid barrier.  Workgroups per replica
 *    and launch: min(work items, 2048 / replicas), a work item being four rows (x) or 256 lines (y, z), and never so few
 *    that a workgroup meets more than 2^30 sites or one work item; no counter of a workgroup passes the sites it meets,
 *    so no 32-bit counter can wrap (csrc/bflbm_chord.h argues the corner).  Expected memory traffic: the field once per
 *    axis, 24 bytes per site and sample.  Then ONE finishing launch, the histogram trace's, writes the totals straight
 *    into the slot [sample][replica][nlevels][W] and sets them back to zero.  No scratch.
 *  - no ring: a z chord crosses the slab boundaries, possibly every one of them, and a slab holds its own planes only.
 *    There is no bflbm_ring_chord_create.  Not built on purpose: chords along diagonals, chords of a second variable, both
 *    sides in one trace, fusing the count into the observation.
 *  - what is touched on the owner: what the morphology trace's observation touches.  The resident state, the step
 *    counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("chord trace
 *    full").  An owner may carry any number of chord traces: rho and phi, or both sides.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched), in this order: null arguments (before any device is touched); the morphology trace's
 *    refusals (nlevels outside 1..8, a non-finite level, a side other than 0 or 1, a source outside 0..1, a component
 *    index outside its source); max_length outside 1..4096; nlevels W above 16384 counters (64 KiB of LDS, the histogram
 *    trace's cap); a plane of more than 2^30 sites; a replica view (use bflbm_batch_chord_create), a context with
 *    nranks > 1; an open step; every < 1, capacity < 1, a capacity beyond 1 TB of records; a failed allocation (the
 *    message gives the bytes of each buffer).  An open step also refuses bflbm_chord_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_chord_read, _count,
 *    _geometry and _destroy still work, bflbm_chord_sample fails.  bflbm_chord_destroy(NULL) returns 0.
 *  - only bflbm_chord_read and bflbm_chord_destroy synchronise the owner's stream. */
typedef struct bflbm_chord bflbm_chord;
int bflbm_chord_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels /* [nlevels] */, int side,
                       int max_length /* M */, int every, long long capacity, bflbm_chord** out);
int bflbm_batch_chord_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side,
                             int max_length, int every, long long capacity, bflbm_chord** out);
int bflbm_chord_destroy(bflbm_chord* t);
int bflbm_chord_sample(bflbm_chord* t);                    /* record the resident state now (e.g. frame 0) */
int bflbm_chord_reset(bflbm_chord* t);                     /* forget the samples, restart the every-counter */
int bflbm_chord_count(const bflbm_chord* t, long long* nsamples, int* nreplicas);
int bflbm_chord_geometry(const bflbm_chord* t, int* nlevels, int* max_length /* M */, int* words /* W */,
                         int* lds_counters /* nlevels W */, int* groups_x, int* groups_y, int* groups_z);
int bflbm_chord_read(bflbm_chord* t, long long first, long long count,
                     long long* counts /* [count][nreplicas][nlevels][W] */,
                     long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Coarse traces: the sums of chosen fields, and of chosen products of them, over the blocks of a window of the box,
 * recorded on the device as a time series of coarse fields and read once at the end.  Every other recorder reduces the
 * observed fields to scalars, profiles, spectra, histograms, counts or tables; this one keeps a field in space over time:
 * the slices and renders of Viewer.ipynb and Visualization.ipynb, a movie of a coarsening mixture or of a droplet that
 * drifts through the box, without downloading hydrovs (22 fields of 8 bytes per site and frame).  With block 1 a sample is
 * a slice or a sub-volume, with block 4 x 4 x 4 a 128^3 movie of a 512^3 box at 1/64 of the bytes; with pairs it carries
 * the block sums of products, from which the block variances and the block-size scaling of the density fluctuations
 * follow, the real-space twin of the flat S(k) of Mixture.ipynb.  A coarse trace is attached to one lone single-slab
 * context or one replica batch.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), nvars in 1..8 distinct component indices of that source, npairs in 0..16 pairs (a, b) of variable SLOTS
 *    (positions in the variable list), a == b allowed, Q = nvars + npairs; a window of the periodic box n = (nx, ny, nz)
 *    by origin[3] (x, y, z), 0 <= o_a < n_a, and extent[3], 1 <= w_a <= n_a: site i of the window along the axis a is
 *    (o_a + i) mod n_a, so a window may run through the seam; block[3] with b_a >= 1, b_a dividing w_a, and b_x <= 256.
 *    The window holds c_a = w_a / b_a blocks along a; block (X, Y, Z) holds the window sites i_a = b_a K_a + d_a,
 *    0 <= d_a < b_a.  A site's term is x_q for q < nvars and x_a * x_b for the pair q - nvars: the product rounded once
 *    and then added, never contracted (-ffp-contract=off), as the profile trace forms its products.  Entry
 *    (q, Z, Y, X) of a sample is the sum of the terms of q over the sites of the block, in this order, which the box,
 *    the window and the block fix alone (never the launch geometry, the batch around a replica, `every`, the capacity,
 *    the schedule, what else is attached, lone context versus replica):
 *      per fine column d_x of the block:   C(d_x) = +0.0;  for d_z = 0 .. b_z-1:  for d_y = 0 .. b_y-1:  C = C + term
 *      then the block:                     S = +0.0;  for d_x = 0 .. b_x-1:  S = S + C(d_x)
 *    These are sums, not means: the reader divides by b_x b_y b_z.  A NaN stays in its block.  With block (1, 1, 1) a
 *    sample is the window itself (a -0.0 reads +0.0).  analysis.coarse_fields restates this in numpy, operation for
 *    operation; analysis.coarse_block_variance turns the sums of a, b and a * b into the covariance within every block.
 *  - sample: [replica][Q][c_z][c_y][c_x] doubles, the variables first, then the pairs.
 *  - bflbm_coarse_geometry reports c_x, c_y, c_z, Q, the fine sites of an x-tile (floor(256 / b_x) b_x), the work items
 *    of a replica (c_z c_y ceil(w_x / x-tile)) and the workgroups of the launch over all replicas.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation,
 *    exactly as the profile trace takes it (a lone context: into the scratch state buffer; a batch: one launch over all
 *    replicas, only the chosen variables, into a buffer of the trace); then ONE launch, compiled once per number of
 *    variables, 256 threads, which writes the slot [sample][replica] directly: no totals, no finishing launch, no
 *    atomics.  A work item is (Z, Y, x-tile): an x-tile is floor(256 / b_x) b_x fine sites of a window row, so no block
 *    straddles a tile.  A lane owns one fine column and marches d_z, d_y with four rows' loads in flight; the lanes lie
 *    along x, so every global load of a wave is a contiguous row segment of 8-byte elements, or two where the wave meets
 *    the seam, never a lane-strided one; a site's variables are loaded once and the products are formed in registers.
 *    After the march the Q column sums pass through LDS once (2048 Q bytes of dynamic LDS, no static LDS) and the first
 *    lane of every block adds its b_x columns left to right and stores.  Work items of at most 64 (128) lanes share a
 *    workgroup four (two) at a time; workgroups per replica: min(turns, 2048 / replicas), a workgroup striding over its
 *    turns.  A block that is tall in y and z is marched by ONE lane per column and a wide one added by one lane: no
 *    chunks, no merge pass; blocks of a few sites per axis are what this is built for.  Expected memory traffic:
 *    8 nvars bytes read per window site and sample, 8 Q / (b_x b_y b_z) written, against the 608 of a step.  The
 *    8-byte loads, the four rows in flight and the 2048 workgroups are untimed heuristics.  No scratch.
 *  - no ring: a block may straddle two slabs, and gathering field-sized blocks onto slab 0 needs a layout decision of its
 *    own.  There is no bflbm_ring_coarse_create.  Not built on purpose: the noise source, output other than doubles,
 *    b_x > 256, a merge pass for tall blocks.
 *  - what is touched on the owner: what the profile trace's observation touches.  The resident state, the step counters
 *    and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("coarse
 *    trace full").  An owner may carry any number of coarse traces: a slice and a coarse volume, say.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched), in this order: null arguments (before any device is touched; pair_a and pair_b may be
 *    NULL only where npairs == 0); a source outside 0..1, nvars outside 1..8, npairs outside 0..16, a component index
 *    outside its source, a repeated variable, a pair slot outside 0..nvars-1; an origin outside 0..n_a-1, then an extent
 *    outside 1..n_a, then per axis a block < 1 or one that does not divide the extent, then b_x > 256; more than 2^30
 *    work items per replica; a replica view (use bflbm_batch_coarse_create), a context with nranks > 1; an open step;
 *    every < 1, capacity < 1; a capacity beyond 1 TB of records; a failed allocation (the message gives the bytes of
 *    each buffer).  An open step also refuses bflbm_coarse_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_coarse_read, _count,
 *    _geometry and _destroy still work, bflbm_coarse_sample fails.  bflbm_coarse_destroy(NULL) returns 0.
 *  - only bflbm_coarse_read and bflbm_coarse_destroy synchronise the owner's stream. */
typedef struct bflbm_coarse bflbm_coarse;
int bflbm_coarse_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs,
                        const int* pair_a /* or NULL if npairs == 0 */, const int* pair_b, const int* origin /* [3]: x, y, z */,
                        const int* extent /* [3] */, const int* block /* [3] */, int every, long long capacity, bflbm_coarse** out);
int bflbm_batch_coarse_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs,
                              const int* pair_a, const int* pair_b, const int* origin, const int* extent, const int* block,
                              int every, long long capacity, bflbm_coarse** out);
int bflbm_coarse_destroy(bflbm_coarse* t);
int bflbm_coarse_sample(bflbm_coarse* t);                  /* record the resident state now (e.g. frame 0) */
int bflbm_coarse_reset(bflbm_coarse* t);                   /* forget the samples, restart the every-counter */
int bflbm_coarse_count(const bflbm_coarse* t, long long* nsamples, int* nreplicas);
int bflbm_coarse_geometry(const bflbm_coarse* t, int* cx, int* cy, int* cz, int* nsums /* Q */, int* tile_sites,
                          int* items /* work items per replica */, int* groups /* workgroups over all replicas */);
int bflbm_coarse_read(bflbm_coarse* t, long long first, long long count,
                      double* sums /* [count][nreplicas][Q][c_z][c_y][c_x] */,
                      long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Lag traces: two-time correlations of chosen fields against time origins kept on the device, recorded as a time
 * series and read once at the end.  Every other recorder reduces the fields of ONE instant.  The velocity autocorrelation
 * sum_x u(x, t0 + lag) . u(x, t0) of an equilibrium run and its long-time tail, the density autocorrelations, the two-time
 * function C(t, t_w) = sum_x phi(x, t) phi(x, t_w) of a quench and the persistence P(t, t_w), the fraction of sites whose
 * side of a level has not changed since t_w, need TWO; the mode trace gives them at up to 64 wavevectors only, and through
 * the host they cost a hydrovs download per sample.  A lag trace keeps per-site copies of earlier samples (origins) on the
 * device and reads them back at every sample.  It is attached to one lone single-slab context or one replica batch.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), nvars in 1..8 distinct component indices of that source, npairs in 1..8 pairs (a, b) of variable SLOTS
 *    (positions in the variable list), a == b allowed, norigins R in 1..16, origin_stride E >= 1, persist_slot (-1 for
 *    none, or a slot in 0..nvars-1) and a finite persist_level.
 *    Origins: the samples are counted n = 0, 1, ... from creation or from the last reset.  At a sample with n % E == 0
 *    the recorder first takes an origin into slot (n / E) % R: it copies the nvars observed variables of every site and
 *    stores the owner's step counter (on a batch each replica's own counter); a used slot is overwritten.  The sample is
 *    then recorded, so every origin appears at lag 0.  The lags covered are 0 to about R E samples.
 *    Sample layout: per replica W = nvars + R (2 + npairs) 8-byte words: now[v], the sum over all sites of variable v at
 *    this sample (double); then per slot r: origin_step[r] (int64, -1 while the slot is empty), alive[r] (int64, -1 if
 *    persist_slot < 0 or the slot is empty) and corr[r][p] = sum_x v_a(x, now) * v_b(x, origin r) (double, NaN for an
 *    empty slot), a the first and b the second slot of pair p.  The product is rounded once and then added, never
 *    contracted (-ffp-contract=off), as the profile trace forms its products.  A NaN in a field propagates.
 *    Persistence: s(v) = (v >= persist_level), an IEEE double comparison: a NaN gives false, a value equal to the level
 *    is above.  Each site has one bit per slot.  A slot's bit is set at every site when its origin is taken; at every
 *    sample, the origin's own sample included, the bit is ANDed with s(v now) == s(v at origin r), v the variable of
 *    persist_slot; alive[r] is the number of set bits.  The bit is checked at samples only, so P depends on `every`: a
 *    site that crosses the level and returns between two samples stays alive.
 *    Order of the double sums: fixed by the box alone.  Per lattice plane z it is the profile trace's axis-z order (tiles
 *    of 2048 consecutive dense sites; thread t of 256 adds the sites t, t + 256, ... in that order, a site past the plane
 *    adding +0.0; then the tree v[t] += v[t + w], w = 128 .. 1; then the tiles are added in tile order from +0.0); after
 *    that the planes are added in the sequence z = 0 .. nz-1, from +0.0.  So now[v] equals the sequential z sum of a
 *    profile trace (axis z) record of the same state, bit for bit, and corr of a just-taken origin equals the same sum
 *    of that trace's pair (a, b).  The integers are exact whatever the launch geometry.  A record does not depend on the
 *    batch around a replica, on the capacity, on the schedule or on what else is attached.  analysis.lag_record restates
 *    this in numpy, operation for operation; analysis.lag_slots is the slot schedule, analysis.lag_average the average
 *    over origins by lag, analysis.lag_connected the connected part.
 *  - bflbm_lag_geometry reports nvars, npairs, R, E, W, the sites of a tile (2048), the tiles of a plane and the bytes of
 *    the origins ([replica][R][nvars][nsites] doubles) and of the masks ([replica][nsites] 16-bit words, 0 without
 *    persistence).
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation,
 *    exactly as the profile trace takes it (a lone context: into the scratch state buffer; a batch: one launch over all
 *    replicas, only the chosen variables, into a buffer of the trace); at a sample that takes an origin one small launch
 *    per 32 replicas that writes the slot's label; then ONE summing launch, compiled once per number of variables, grid
 *    (tiles of a plane, planes, replicas), 256 threads: a thread loads the current values of its 8 turns once (16-byte
 *    loads where the plane is aligned) and keeps them in registers, adds them into now, stores them into the slot that
 *    takes an origin (whose products then use the registers), and loops over the live slots with the origin's values
 *    streaming through: per slot and pair one per-thread sum, the tree, one partial per (plane, tile, slot, pair).  With
 *    persistence it loads the site's 16-bit mask once, updates every live bit from the values in registers and stores it;
 *    the set bits are counted by wave ballots, one LDS add per wave and slot, one 64-bit global integer add per non-zero
 *    counter and workgroup.  Two small finishing launches: the tiles of a plane in order; then the planes in sequence,
 *    the counters and the origin labels into the slot [sample][replica][W], and the counters back to zero.  No atomics
 *    on doubles, no scratch, no grid barrier.  Expected memory traffic per site and sample, derived: 8 nvars (1 + L)
 *    bytes read, L the live slots, 8 nvars written at an origin sample, 4 for the mask: 408 bytes with three velocity
 *    components and 16 origins, against the 608 of a step.
 *  - no ring: there is no bflbm_ring_lag_create.  It would be easy later (per-site data stays on its slab, and the
 *    partials gather in plane order as the profile trace's do); it is not built.  Not built on purpose either: the noise
 *    source, more than 16 origins, logarithmically spaced origins, per-site lagged products.
 *  - what is touched on the owner: what the profile trace's observation touches.  The resident state, the step counters
 *    and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("lag trace
 *    full").  bflbm_lag_reset also empties the slots and restarts n.  An owner may carry any number of lag traces.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched), in this order: null arguments (before any device is touched); a source outside 0..1,
 *    nvars outside 1..8, npairs outside 1..8, a component index outside its source, a repeated variable, a pair slot
 *    outside 0..nvars-1; R outside 1..16, E < 1, persist_slot outside -1..nvars-1, a non-finite level when a slot is
 *    given; every < 1, capacity < 1, a capacity beyond 1 TB of records; a replica view (use bflbm_batch_lag_create), a
 *    context with nranks > 1; an open step; more than 65535 planes; a failed allocation (the message gives the bytes of
 *    the origins, the masks, the stage buffer and the records).  An open step also refuses bflbm_lag_sample, _reset and
 *    _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_lag_read, _count,
 *    _geometry and _destroy still work, bflbm_lag_sample fails.  bflbm_lag_destroy(NULL) returns 0.
 *  - only bflbm_lag_read and bflbm_lag_destroy synchronise the owner's stream. */
typedef struct bflbm_lag bflbm_lag;
int bflbm_lag_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                     int norigins, int origin_stride, int persist_slot /* or -1 */, double persist_level, int every,
                     long long capacity, bflbm_lag** out);
int bflbm_batch_lag_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs, const int* pair_a, const int* pair_b,
                           int norigins, int origin_stride, int persist_slot, double persist_level, int every,
                           long long capacity, bflbm_lag** out);
int bflbm_lag_destroy(bflbm_lag* t);
int bflbm_lag_sample(bflbm_lag* t);                        /* record the resident state now (e.g. frame 0) */
int bflbm_lag_reset(bflbm_lag* t);                         /* forget the samples and the origins, restart both counters */
int bflbm_lag_count(const bflbm_lag* t, long long* nsamples, int* nreplicas);
int bflbm_lag_geometry(const bflbm_lag* t, int* nvars, int* npairs, int* norigins, int* origin_stride, int* words /* W */,
                       int* tile_sites, int* tiles_per_plane, long long* origin_bytes, long long* mask_bytes);
int bflbm_lag_read(bflbm_lag* t, long long first, long long count,
                   double* words /* [count][nreplicas][W] 8-byte words, copied bit for bit: doubles and int64 */,
                   long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Moment traces: the box sums of all 19 kinetic moments of both fluids, of their squares and of the products of the two
 * fluids' moments mode by mode, recorded as a time series and read once at the end.  The thermal noise is applied per mode,
 * to all 19 moments of each fluid (LBM_binary.H:73-132); every other recorder reads hydrovs, hydrovsbar or the injected
 * noise moments, and of the moments m = M f of the resident state only density and momentum ever leave the step.  Whether
 * all modes are thermalised (equipartition per mode), the box sum of the off-diagonal stress that a Green-Kubo integral
 * needs at every step, and whether the two fluids' kinetic modes fluctuate together or against each other otherwise cost
 * a download of 38 populations per site and sample.  A moment trace is attached to one lone single-slab context or one
 * replica batch.
 *  - definition (stated here and nowhere else).  No inputs besides the cadence: there are no variable lists and no pair
 *    lists.  At every site mf = moments(f) and mg = moments(g), f and g the populations that bflbm_download_fg returns (the
 *    reference's fold / gold) and moments the transform of LBM_d3q19.H:100-156 with the association of its expressions, so
 *    the doubles are those the step's own collision forms.  Global moment index i = 19 fluid + a, fluid 0 (f) or 1 (g),
 *    a = 0..18: the numbering of the noise source (fa0..fa18, ga0..ga18).
 *    Sample layout: per replica W = 95 doubles: sum[i] (words 0..37) = sum over all sites x of m_i(x); sq[i] (words
 *    38..75) = sum_x m_i(x) * m_i(x); cross[a] (words 76..94) = sum_x mf_a(x) * mg_a(x), a = 0..18.  Every product is
 *    rounded once and then added, never contracted (-ffp-contract=off), as the profile trace forms its products.  A NaN
 *    stays in its sum: it shows in exactly the words its moments enter.
 *    Order of every sum: the lag trace's order for `now` ("Lag traces", Order of the double sums), with m_i, m_i * m_i or
 *    mf_a * mg_a in the place of the variable.  So the record depends on the box alone: it is reproducible bit for bit,
 *    independent of the schedule in force, of the batch around a replica, of the capacity and of what else is attached.
 *    analysis.moment_record restates this in numpy, operation for operation;
 *    analysis.moment_names names the modes, analysis.moment_variances, analysis.equipartition and analysis.stress_series
 *    cut a record up.
 *  - bflbm_moment_geometry reports W (95), the sites of a tile (2048) and the tiles of a plane.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: ONE summing launch, grid (tiles of
 *    a plane, planes, replicas), 256 threads, which takes a lone context by its resident buffer and a batch by the
 *    replicas' records: per site the pull of the 38 populations, the transform twice, 95 accumulators in registers, every
 *    one with a compile-time index; the tree 12 accumulators at a time through two LDS buffers in turn (49152 bytes of
 *    static LDS); one partial per (word, tile): [replica][z][95][tiles].  One finishing launch, grid (95, replicas): the
 *    tiles of every plane in tile order, then the planes in sequence, straight into the slot [sample][replica][95].
 *    No atomics, no scratch, no
 *    grid barrier.  Expected memory traffic per site and sample, derived: 304 bytes read against the 608 of a step,
 *    nothing written but 95 x tiles partials per plane.
 *  - no ring: there is no bflbm_ring_moment_create.  It would be easy later (the summing launch takes a slab as it takes a
 *    lone context, and the partials gather in plane order as the profile trace's do); it is not built.
 *  - not built on purpose: a source in the field selection, per-site output, density-normalised or windowed sums, the
 *    deviation from the local equilibrium, arbitrary pairs of modes, a Green-Kubo integral.
 *  - what is touched on the owner: nothing.  The resident state is read; the scratch state buffer, the densities, the
 *    step counters and the noise index are neither written nor moved.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("moment
 *    trace full").  An owner may carry any number of moment traces.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched), in this order: null arguments (before any device is touched); every < 1, capacity < 1, a
 *    capacity beyond 1 TB of records; a replica view (use bflbm_batch_moment_create), a context with nranks > 1; an open step; more than 65535 planes, a plane beyond a 32-bit site index,
 *    more than 65535 replicas; a failed allocation.  An open step also refuses bflbm_moment_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_moment_read, _count,
 *    _geometry and _destroy still work, bflbm_moment_sample fails.  bflbm_moment_destroy(NULL) returns 0.
 *  - only bflbm_moment_read and bflbm_moment_destroy synchronise the owner's stream. */
typedef struct bflbm_moment bflbm_moment;
int bflbm_moment_create(bflbm_ctx* c, int every, long long capacity, bflbm_moment** out);
int bflbm_batch_moment_create(bflbm_batch* b, int every, long long capacity, bflbm_moment** out);
int bflbm_moment_destroy(bflbm_moment* t);
int bflbm_moment_sample(bflbm_moment* t);                  /* record the resident state now (e.g. frame 0) */
int bflbm_moment_reset(bflbm_moment* t);                   /* forget the samples and restart the every-counter */
int bflbm_moment_count(const bflbm_moment* t, long long* nsamples, int* nreplicas);
int bflbm_moment_geometry(const bflbm_moment* t, int* words /* W = 95 */, int* tile_sites, int* tiles_per_plane);
int bflbm_moment_read(bflbm_moment* t, long long first, long long count,
                      double* sums /* [count][nreplicas][95] */,
                      long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Cluster traces: the connected components of a thresholded field, labelled on the device by a union-find over the
 * lattice and recorded as a time series of 64-bit integers, read once at the end.  The morphology trace answers "how many
 * domains" only through chi, which is the count only while no domain has a tunnel or a cavity, and never gives a size.
 * This one records the number of components, the size of the largest, the sum of the squared sizes and a histogram of the
 * sizes in powers of two: the droplet-size distribution of an off-critical quench, the mass fraction of the largest domain
 * (the order parameter of the bicontinuous-to-droplet transition), a satellite that has pinched off in one replica of a
 * batch; bflbm_cluster_labels hands out which sites belong to which component.  A cluster trace is attached to one lone
 * single-slab context or one replica batch.
 *  - definition (stated here and nowhere else).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9
 *    components), one component index v of that source, nlevels in 1..8 finite levels t_l, a side with the morphology
 *    trace's semantics (side 0 occupies the site (x, y, z) at level l when v[z][y][x] >= t_l, side 1 when v[z][y][x] < t_l;
 *    IEEE double comparisons: a NaN occupies nothing on either side, -0.0 equals +0.0) and a connectivity, 6 (faces) or 26
 *    (faces, edges and corners: the closed-voxel union of the morphology trace, so that for tunnel-free domains
 *    ncomp == chi).  Links: two occupied sites are linked where one is the periodic neighbour of the other along one of
 *    the 3 (connectivity 6) or 13 (connectivity 26) forward directions (dx, dy, dz) in {-1, 0, 1}^3 with (dz, dy, dx)
 *    lexicographically positive, coordinates modulo the extents.  This holds on extents 1 and 2 as it stands: a site that
 *    is its own neighbour, or whose + and - neighbours coincide, neither creates nor removes a component.  A component is a
 *    class of the transitive closure of the links.  The canonical label of an occupied site is the smallest linear index
 *    p = (z ny + y) nx + x of its component, the label of an unoccupied site -1.  Labels are 32-bit: nx ny nz > 2^31 - 1 is
 *    refused.  analysis.cluster_labels and analysis.cluster_record restate the rule in numpy.
 *  - sample: [replica][nlevels][W] 64-bit signed integers with W = 38, per level in the order of the levels:
 *      word 0        ncomp, the number of components
 *      word 1        V, the number of occupied sites (the morphology trace's N3)
 *      word 2        smax, the size of the largest component (0 if none)
 *      word 3        the label of the largest component; among equals the smallest label; -1 if none
 *      word 4        the sum of s^2 over the components (it fits: sum s^2 <= V^2 <= 2^62)
 *      word 5        capped: device loops that hit their iteration cap (below); 0 in every correct run
 *      word 6 + b    b = 0..31: the components with 2^b <= s < 2^(b+1)
 *    All are integers: a record does not depend on the number of replicas, `every`, the capacity, the schedule, what else
 *    is attached, lone context versus replica, or the launch geometry.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation of
 *    the one variable, exactly as the morphology trace takes it; then per level, one after another through the same two
 *    32-bit arrays parent and size [replica][nsites], 4 launches: k_cluster_local, one workgroup of 256 threads per brick of
 *    32 x 4 x 4 sites (an untimed heuristic), unites in LDS the links inside the brick that do not wrap and writes every
 *    site's brick-local root and every local root's size; k_cluster_merge unites in global memory every link that crosses
 *    a brick face or wraps (those of a brick with itself included) in the lock-free form: find both roots, an atomic
 *    minimum of the larger root's parent with the smaller, go on from the value returned if that root had meanwhile been
 *    linked; k_cluster_resolve lets every brick-local root find its global root and add its size to it, so that the adds
 *    per component are the bricks it touches, not its sites; k_cluster_stats sums words 0, 1, 4 and the bins over the global
 *    roots per wave and workgroup (one 64-bit global add per non-zero counter and workgroup) and takes words 2 and 3 as one
 *    packed 64-bit maximum, (size << 32) | (0xffffffff - label).  Then ONE finishing launch, k_cluster_finish, writes the
 *    totals of all levels into the slot, unpacks the maximum and clears the totals.  The phases are separated by launches:
 *    no grid barrier, no persistent kernel.  A root is always the smallest index of its tree (parent[p] <= p throughout).
 *    Inside the merge and resolve launches the parents are read with relaxed agent-scope atomic loads and written with
 *    agent-scope atomic minima only: parents only decrease, a stale parent is an older ancestor of the same tree, and
 *    every link is decided by the value an atomic returns (csrc/bflbm_cluster.h argues it in full).
 *  - termination: a find follows strictly falling indices and a union replaces the larger site of its pair by a smaller
 *    one, so both end within nsites turns; both loops carry nsites as a hard cap as well, and a loop that reaches it adds
 *    one to word 5 and leaves: a defect shows as capped != 0, never as a hang.  No scratch; static LDS 4096 bytes
 *    (k_cluster_local) and 152 bytes (k_cluster_stats).
 *  - memory per trace: parent and size, 8 bytes per site and replica; a batch also the dense field, 8 bytes per site and
 *    replica, as the morphology trace.
 *  - bflbm_cluster_geometry reports nlevels, the connectivity, the brick extents (32, 4, 4), the bricks per replica and
 *    the launches per level (4).
 *  - bflbm_cluster_labels labels the owner's resident state now, for the level level_index: the observation, the local and
 *    merge launches and one flatten launch that reads the parents only and writes every site's root into the size array;
 *    it synchronises and writes the canonical labels [replica][nz][ny][nx] as 32-bit integers.  It records no sample and
 *    leaves the trace's totals and every-count untouched.  Refused: null arguments, a level index outside the levels, a
 *    detached trace, an open step, a loop that hit its cap.
 *  - out of scope: rings (a link crosses the slab boundary and needs the next slab's parents; there is
 *    no bflbm_ring_cluster_create, the morphology trace's exclusion), per-component sums of a second variable, wrapping
 *    (winding) detection, component tracking on the device, 18-connectivity, a noise source.  Per-component size, origin,
 *    extent (spanning), integer moments and area are the component trace's ("Component traces" below).
 *  - what is touched on the owner: what the morphology trace's observation touches.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces
 *    ("cluster trace full").  An owner may carry any number of cluster traces.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments (before any device is touched), then the morphology trace's refusals in its
 *    order and wording (nlevels outside 1..8, a non-finite level, a side other than 0 or 1, a source outside 0..1, a
 *    component index outside its source), "connectivity must be 6 or 26 (got %d)", every < 1, capacity < 1, a replica view
 *    (use bflbm_batch_cluster_create), a context with nranks > 1, an open step, more than 2^31 - 1 sites, a capacity beyond
 *    1 TB of records, a failed allocation (the message gives the bytes of each buffer).  An open step also refuses
 *    bflbm_cluster_sample, _reset, _read and _labels.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_cluster_read, _count,
 *    _geometry and _destroy still work, bflbm_cluster_sample and _labels fail.  bflbm_cluster_destroy(NULL) returns 0.
 *  - only bflbm_cluster_read, bflbm_cluster_labels and bflbm_cluster_destroy synchronise the owner's stream. */
typedef struct bflbm_cluster bflbm_cluster;
int bflbm_cluster_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels /* [nlevels] */, int side,
                         int connectivity, int every, long long capacity, bflbm_cluster** out);
int bflbm_batch_cluster_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side,
                               int connectivity, int every, long long capacity, bflbm_cluster** out);
int bflbm_cluster_destroy(bflbm_cluster* t);
int bflbm_cluster_sample(bflbm_cluster* t);                /* record the resident state now (e.g. frame 0) */
int bflbm_cluster_reset(bflbm_cluster* t);                 /* forget the samples, restart the every-counter */
int bflbm_cluster_count(const bflbm_cluster* t, long long* nsamples, int* nreplicas);
int bflbm_cluster_geometry(const bflbm_cluster* t, int* nlevels, int* connectivity, int* brick_x, int* brick_y, int* brick_z,
                           int* bricks /* per replica */, int* launches /* per level */);
int bflbm_cluster_read(bflbm_cluster* t, long long first, long long count,
                       long long* counts /* [count][nreplicas][nlevels][38] */,
                       long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);
int bflbm_cluster_labels(bflbm_cluster* t, int level_index, int* labels /* [nreplicas][nz][ny][nx] */);

/* ---- Component traces: per connected component of a thresholded field its size, where it is, how far it reaches along
 * every axis, the integer first and second moments of its sites and its area, recorded on the device as a time series of
 * 64-bit integers and read once at the end.  The cluster trace reduces the components to one record per level; the
 * ensemble trace gives one centre for the whole box, which means nothing with two droplets in it.  This one tabulates
 * the droplets of an off-critical quench or a many-droplet box: centroid, gyration tensor and interface area of each,
 * whether a domain has reached across the box, and, through analysis.track_components, per-droplet trajectories for
 * analysis.msd.  A component trace is attached to one lone single-slab context or one replica batch.
 *  - definition (stated here and nowhere else).  Inputs: the cluster trace's (a source, one component index v, nlevels in
 *    1..8 finite levels, a side, a connectivity 6 or 26, with its semantics), min_size >= 1 (64-bit) and rows in 1..256.
 *    Per replica and level the components and their canonical labels are exactly the cluster trace's: the label of a
 *    component is the smallest linear index p = (z ny + y) nx + x of its sites.  A component qualifies when its size is
 *    >= min_size.  The qualifying components are ranked by ascending label: row j belongs to the qualifying component with
 *    j qualifying components of smaller label.  Rows >= rows are dropped and the header says so (nqual > nrows).
 *    Arc: neighbouring sites differ by at most 1 per coordinate (modulo the extent) under either connectivity, so the
 *    projection of a connected component on an axis is connected on the periodic axis: a single arc, or all of it.
 *    Per axis a of extent n_a: extent_a is the number of occupied coordinates; origin_a is the one occupied coordinate
 *    whose predecessor (c - 1) mod n_a is unoccupied; where every coordinate is occupied the origin is 0 and the component
 *    SPANS the axis (extent_a == n_a; an axis of extent 1 is always spanned).  With d_a = (c_a - origin_a) mod n_a over the
 *    component's sites, unwrapping a non-spanning axis from the origin is unambiguous: the sums below are those of the
 *    unwrapped component wherever it lies across the periodic planes.  Spanning is necessary for wrapping (a closed path
 *    of links that winds around the axis), not sufficient: a path may cover every x without a link across the x plane.
 *    Nothing here detects wrapping.  Faces: the number of pairs (site of the component, one of the 6 axis directions)
 *    whose periodic neighbour is unoccupied; on an axis of extent 2 the + and - neighbour are the same site and count
 *    twice, on extent 1 the neighbour is the site itself.  Summed over all components this is the morphology trace's
 *    S = -6 N3 + 2 N2 at the same level and side: every occupied site counts its unoccupied neighbours, 6 N3 minus the
 *    ordered occupied pairs along the axes; per axis [o | o+] = o + o+ - o o+ gives N2 = 6 N3 - P with P the unordered
 *    pairs, so the ordered pairs are 2 P = 12 N3 - 2 N2.
 *    analysis.component_table restates the rule in numpy.
 *  - sample: [replica][nlevels][6 + rows x 18] 64-bit signed integers, per level the header, then the rows:
 *      header word 0   ncomp, the number of components            (the cluster trace's word 0)
 *      header word 1   V, the number of occupied sites             (the cluster trace's word 1)
 *      header word 2   nqual, the qualifying components
 *      header word 3   Vqual, the sites in all qualifying components, tabulated or not
 *      header word 4   nrows = min(nqual, rows)
 *      header word 5   capped, the cluster trace's word 5: 0 in every correct run
 *      row word 0      label               row words 2-4    origin (ox, oy, oz)      row words 5-7    extent (ex, ey, ez)
 *      row word 1      size                row words 8-10   sum dx, sum dy, sum dz   row words 11-13  sum dx^2, dy^2, dz^2
 *      row word 17     faces               row words 14-16  sum dx dy, sum dx dz, sum dy dz
 *    Unused rows (j >= nrows) have label -1 and zeros elsewhere.  All are integers: a record does not depend on the number
 *    of replicas, `every`, the capacity, the schedule, what else is attached, lone context versus replica, the launch
 *    geometry or the order in which atomics land.
 *  - overflow: an extent above 65536 is refused, so d_a d_b < 2^32, and nsites <= 2^31 - 1 bounds every sum of a component
 *    by 2^31 2^32 = 2^63 (for a != b already d_a d_b < n_a n_b <= nsites).  No 32-bit accumulator holds a sum that can
 *    exceed it: a brick's partial sums in LDS reach 512 x 2^32 and are 64-bit (csrc/bflbm_components.h argues it); the
 *    32-bit counters count sites or roots of one workgroup (<= 1024) or qualifying roots (< 2^31).
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the cluster trace's observation;
 *    then per level, one after another, 9 launches: k_cluster_local, k_cluster_merge and k_cluster_resolve, the cluster
 *    trace's own, after which a site reaches its global root in two plain loads (its brick-local root, then that root's
 *    parent); k_component_count, k_component_scan and k_component_rank, a deterministic exclusive prefix count of the
 *    qualifying roots in label order (per workgroup of 1024 sites, over the workgroups, inside the workgroup), which sums
 *    header words 0..3, writes label and size into rows < rows and leaves every global root its slot or -1;
 *    k_component_masks, one workgroup per brick of 32 x 4 x 4 sites, ORs the brick's coordinate bits per component in LDS
 *    and flushes one 64-bit atomic OR per (component present in the brick, axis); k_component_origin turns the masks into
 *    origin and extent per (replica, slot, axis) and clears them; k_component_moments, one workgroup per brick,
 *    accumulates the 9 sums and the faces per component in LDS with 64-bit LDS atomics and flushes 64-bit global adds per
 *    (component present in the brick): the global atomics per component are the bricks it touches, not its sites.  Then
 *    ONE finishing launch, k_component_finish, writes header and rows of all levels into the slot and clears the staging.
 *    The phases are separated by launches: no grid barrier.  What a launch reads of an earlier launch it reads with plain
 *    loads; inside a launch a word another workgroup may touch is only ever the target of an agent-scope atomic
 *    read-modify-write and is not read back.  The new kernels follow no parent chains; the loops of the three labelling
 *    launches carry the cluster trace's hard cap and count into header word 5.  No scratch; static LDS 24, 16, 64, 6144, 0,
 *    43008 and 0 bytes (count, scan, rank, masks, origin, moments, finish).
 *  - memory per trace: parent and size, 8 bytes per site and replica (a global root's size word becomes its slot); a batch
 *    also the dense field, 8 bytes per site and replica; per replica rows x (ceil(nx / 64) + ceil(ny / 64) + ceil(nz / 64))
 *    mask words and 4 bytes per 1024 sites.  Traffic per site and level, derived, not measured: about 50 bytes (24 of the
 *    labelling, 16 of count and rank, 4 + 4 of the two brick launches plus re-loads through the caches) against the 608 of
 *    a step.
 *  - bflbm_component_geometry reports nlevels, the connectivity, min_size, rows, the header words (6), the row words (18)
 *    and the launches per level (9).
 *  - out of scope: mass-weighted or second-variable sums per component (a float sum per component has no fixed order
 *    under atomics), true wrapping (winding) detection, tracking on the device (analysis.track_components links the rows
 *    of consecutive samples on the host), rings (no bflbm_ring_component_create, the cluster trace's exclusion),
 *    18-connectivity.
 *  - what is touched on the owner, sampling rule, capacity, step labels, order among the recorders of one owner: those of
 *    the cluster trace ("component trace full").  An owner may carry any number of component traces.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments (before any device is touched), then the cluster trace's refusals in its
 *    order and wording up to the connectivity, "min_size must be >= 1 (got %lld)", "rows must be in 1..256 (got %d)",
 *    every < 1, capacity < 1, a replica view (use bflbm_batch_component_create), a context with nranks > 1, an open step,
 *    more than 2^31 - 1 sites, an extent above 65536, a capacity beyond 1 TB of records, a failed allocation (the message
 *    gives the bytes of each buffer).  An open step also refuses bflbm_component_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_component_read, _count,
 *    _geometry and _destroy still work, bflbm_component_sample fails.  bflbm_component_destroy(NULL) returns 0.
 *  - only bflbm_component_read and bflbm_component_destroy synchronise the owner's stream. */
typedef struct bflbm_component bflbm_component;
int bflbm_component_create(bflbm_ctx* c, int source, int var, int nlevels, const double* levels /* [nlevels] */, int side,
                           int connectivity, long long min_size, int rows, int every, long long capacity,
                           bflbm_component** out);
int bflbm_batch_component_create(bflbm_batch* b, int source, int var, int nlevels, const double* levels, int side,
                                 int connectivity, long long min_size, int rows, int every, long long capacity,
                                 bflbm_component** out);
int bflbm_component_destroy(bflbm_component* t);
int bflbm_component_sample(bflbm_component* t);            /* record the resident state now (e.g. frame 0) */
int bflbm_component_reset(bflbm_component* t);             /* forget the samples, restart the every-counter */
int bflbm_component_count(const bflbm_component* t, long long* nsamples, int* nreplicas);
int bflbm_component_geometry(const bflbm_component* t, int* nlevels, int* connectivity, long long* min_size, int* rows,
                             int* header_words, int* row_words, int* launches /* per level */);
int bflbm_component_read(bflbm_component* t, long long first, long long count,
                         long long* record /* [count][nreplicas][nlevels][6 + rows x 18] */,
                         long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* ---- Radial traces: the sums of chosen fields, of chosen products of them and of chosen projections onto the outward
 * radial unit vector, over the shells of width delta about a droplet's centre, recorded on the device as a time series
 * and read once at the end.  Surface_Tension.ipynb's droplet route needs, per droplet, the pressure inside and outside
 * (cell 13: p = rhot cs2 + alpha0 cs2 rho phi), the Shan-Chen force rho af + phi ag integrated from the edge to the
 * centre, and a radius, and regresses Delta p against 1 / R; Droplet_Fluctuation.ipynb fits tanh profiles of rho(r) per
 * frame.  Under thermal noise a single lattice line is useless; the shell average about the moving centre is what one
 * wants, and it is a few dozen numbers (analysis.radial_pressure, pressure_jump, radial_force_integral,
 * fit_radial_profile, equimolar_radius).  A radial trace is the profile trace turned from planes into shells; it is
 * attached to one lone single-slab context or one replica batch (no rings: droplet ensembles are small boxes).
 *  - definition (stated here and nowhere else).  Every operation is an IEEE double operation in the stated order, never
 *    contracted (-ffp-contract=off).  Inputs: a source (0: hydrovs, 22 components; 1: hydrovsbar, 9 components), nvars in
 *    1..8 distinct component indices of that source, npairs in 0..16 pairs (a, b) of variable SLOTS (positions in the
 *    variable list), a == b allowed, nrad in 0..4 radial terms (w, vx, vy, vz) of variable slots, w a slot or -1, either a
 *    fixed centre c[3] in cell-index coordinates (one for all replicas) or a null centre with a threshold, a shell width
 *    delta > 0 in cells and nbins in 1..128.  The null centre is the shape trace's rule: the same kernels in the same
 *    order, so c_a = record 1 + a / record 0 of bflbm_trace_read of the same state and threshold bit for bit, NaN where
 *    no cell is above the threshold.
 *    Site geometry: for the site (ix, iy, iz) and per axis a, d_a = (double)i_a - c_a; h_a = 0.5 * (double)n_a; if
 *    d_a >= h_a then d_a = d_a - (double)n_a, else if d_a < -h_a then d_a = d_a + (double)n_a (the minimum image).
 *    r = sqrt((dx*dx + dy*dy) + dz*dz); q = r / delta; the site belongs to shell k = (int)q if q < (double)nbins and to
 *    no shell otherwise, a NaN q included.
 *    Terms of a site, Q = nvars + npairs + nrad: x_q for a variable; x_a * x_b for a pair; for a radial term
 *    p = ((x_vx*dx + x_vy*dy) + x_vz*dz) / r, p = +0.0 where r == 0, and the term is p for w = -1, else x_w * p; the
 *    count term is 1.0.  analysis.radial_shells restates this in numpy, operation for operation and in the order below.
 *  - order of a sum, fixed by the box alone.  Every sum starts from +0.0.  The dense plane z (sites s = y nx + x) is cut
 *    into tiles of 256 consecutive sites, the last one short.  The partial of (term, shell, tile) adds the terms of the
 *    tile's member sites sequentially in ascending s; the partials of a plane are added in tile order; the planes are
 *    added in the sequence z = 0 .. nz-1.  A partial with no member site is +0.0 and no sum from +0.0 is ever -0.0, so
 *    leaving it out changes no bit: the implementation skips empty shells and tiles.  No atomics.  A record does not
 *    depend on the number of replicas, `every`, the capacity, the schedule, what else is attached, or lone context
 *    versus replica.  bflbm_radial_geometry reports Q, nbins, the sites of a tile (256) and the tiles per plane.
 *  - sample: [replica][3 + (1 + Q) nbins] doubles: the centre used (cx, cy, cz), the counts [nbins], then the sums
 *    [Q][nbins], variables first, then pairs, then radial terms.  These are sums: the reader divides by the counts.
 *  - how a sample is taken, on the owner's stream and without a host synchronisation: the accumulators' observation,
 *    exactly as the profile trace takes it (a lone context: into the scratch state buffer; a batch: one launch over all
 *    replicas, only the chosen variables, into a buffer of the trace); with a null centre the two ensemble-trace
 *    kernels into a buffer of the trace; the shell kernel, one workgroup of 256 threads per (replica, plane), compiled
 *    once per number of variables, which walks its tiles in order: per tile every thread loads its site's variables
 *    (8-byte loads, a wave reads 512 contiguous bytes per variable), forms d, r, the shell and the projections and stages
 *    the variables, the projections and the shell in LDS (2048 (nvars + 4) + 1312 bytes); the tile's lowest and highest
 *    shell come from an integer reduction; thread t owns the items (shell, term) = divmod(t + 256 j, 1 + Q), j = 0, 1,
 *    ..., and for those inside the tile's shell range walks the tile's sites in order and adds the members' terms,
 *    products formed on the fly from the staged rows, then adds the tile's partial to its per-plane accumulator in a
 *    register; one [1 + Q][nbins] block per (replica, plane) leaves the kernel; then the finishing launch, one thread per
 *    (replica, term, shell), adds the planes in sequence straight into the slot [sample][replica] and writes the centre.
 *    No atomics, no scratch.  The tile size and the item-to-thread map are untimed heuristics.
 *  - what is touched on the owner: what the profile trace's observation touches.  Observing hydrovs rewrites rho / phi by
 *    the density pass where they are stale; a context's scratch state buffer is overwritten.  The resident state, the
 *    step counters and everything the owner computes are unchanged.
 *  - sampling rule, capacity, step labels, order among the recorders of one owner: those of the other traces ("radial
 *    trace full").  An owner may carry any number of radial traces.
 *  - not covered: a droplet that diffuses across the periodic boundary.  The centre is the ensemble trace's, which does
 *    not unwrap, while the shells use the minimum image.
 *  - refused at creation (non-zero return, a message naming the call, before any launch, nothing allocated, the owner's
 *    recorder list untouched): null arguments, a source outside 0..1, nvars outside 1..8, npairs outside 0..16, nrad
 *    outside 0..4, a repeated variable, a component index outside its source, a pair or radial slot outside
 *    0..nvars-1 (w = -1 excepted), a non-finite fixed centre, a NaN threshold with a null centre, a delta that is not
 *    finite or <= 0, nbins outside 1..128, every < 1, capacity < 1, a capacity beyond 1 TB of records, nz > 65535, a
 *    replica view (use bflbm_batch_radial_create), a context with nranks > 1, an open step, a failed allocation.  An
 *    open step also refuses bflbm_radial_sample, _reset and _read.
 *  - lifetime: the trace owns its buffers.  Destroying the owner first detaches the trace: bflbm_radial_read, _count,
 *    _geometry and _destroy still work, bflbm_radial_sample fails.  bflbm_radial_destroy(NULL) returns 0.
 *  - only bflbm_radial_read and bflbm_radial_destroy synchronise the owner's stream. */
typedef struct bflbm_radial bflbm_radial;
int bflbm_radial_create(bflbm_ctx* c, int source, int nvars, const int* vars, int npairs,
                        const int* pair_a /* or NULL if npairs == 0 */, const int* pair_b,
                        int nrad, const int* rad_w /* [nrad], or NULL if nrad == 0 */, const int* rad_v /* [nrad][3] */,
                        const double* centre_or_null /* [3] */, double threshold, double delta, int nbins,
                        int every, long long capacity, bflbm_radial** out);
int bflbm_batch_radial_create(bflbm_batch* b, int source, int nvars, const int* vars, int npairs,
                              const int* pair_a, const int* pair_b, int nrad, const int* rad_w, const int* rad_v,
                              const double* centre_or_null, double threshold, double delta, int nbins,
                              int every, long long capacity, bflbm_radial** out);
int bflbm_radial_destroy(bflbm_radial* t);
int bflbm_radial_sample(bflbm_radial* t);                  /* record the resident state now (e.g. frame 0) */
int bflbm_radial_reset(bflbm_radial* t);                   /* forget the samples, restart the every-counter */
int bflbm_radial_count(const bflbm_radial* t, long long* nsamples, int* nreplicas);
int bflbm_radial_geometry(const bflbm_radial* t, int* nsums /* Q */, int* nbins, int* tile_sites, int* tiles_per_plane);
int bflbm_radial_read(bflbm_radial* t, long long first, long long count,
                      double* rec /* [count][nreplicas][3 + (1 + Q) nbins] */,
                      long long* steps /* [count][nreplicas], nullable: each replica's step counter at the sample */);

/* Materialise the per-step fields the reference keeps in MultiFabs, for the state
 * after the last completed step:
 *   hydrovsbar comps 0..8  (LBM_hydrovars_density, LBM_binary.H:315-354)
 *   fnoisevs/gnoisevs      (thermal_noise, :73-132)
 *   hydrovs comps 0..ncomp-1 <= 22 (LBM_hydrovars, :196-313; legacy drivers pass 15)
 * Each destination is a host FAB of `box` with the stated number of components;
 * NULL skips that field. */
int bflbm_get_hydrovsbar(bflbm_ctx* c, double* dst, int ncomp, const bflbm_fab* box);
int bflbm_get_hydrovs(bflbm_ctx* c, double* dst, int ncomp, const bflbm_fab* box);
int bflbm_get_noise(bflbm_ctx* c, double* fnoise, double* gnoise, const bflbm_fab* box);

/* Test hook: feed the collision of the NEXT step with these noise moments instead of
 * the built-in generator (the reference's RNG stream is not reproducible).
 * Pass NULL,NULL to return to the generator.
 * The injected moments stand where the reference keeps fnoisevs / gnoisevs of the resident state, so:
 *  - until that step ran, bflbm_get_noise returns them and bflbm_get_hydrovs is computed with them (LBM_hydrovars reads
 *    modes 1..3, :298-313), and no schedule resolves to 3;
 *  - they feed ONE step: the steps after it draw generated noise again;
 *  - a new resident state drops them: every LBM_init_* and LBM_init draws the noise of the state it made (:625, :654,
 *    :691, :740), so bflbm_init_*, bflbm_commit_upload (with either reset_step_counter) and bflbm_tune_placement end a
 *    pending injection;
 *  - what leaves the state alone keeps them: bflbm_set_step_count, bflbm_set_params, bflbm_set_schedule and every
 *    observable. */
int bflbm_inject_noise(bflbm_ctx* c, const double* fnoise, const double* gnoise, const bflbm_fab* box);

/* update_com (LBM_hydrovs.H:26-60) over this slab: sums of rho, rho*i, rho*j, rho*k
 * (4 doubles; the caller all-reduces across slabs and divides). */
int bflbm_com_sums(bflbm_ctx* c, double sums[4]);

/* Total of rho and phi over the slab (PrintMassConservation, Debug.H:232-249). */
int bflbm_mass(bflbm_ctx* c, double* rho_sum, double* phi_sum);

/* ---- Reference-state noise: the reference's compile-time USE_REF_STATE branch (LBM_binary.H:12,
 * :92-107) as a run-time switch.  The noise amplitudes of thermal_noise are then taken from the
 * equilibrium fields rho_eq, phi_eq, rhot_eq (main_run_job.cpp:216-235) at the site shifted by
 * static_cast<int>(COM - com_ref), COM = update_com of the state the noise belongs to
 * (LBM_binary.H:585-590).  Like the reference's callers, the state left by bflbm_init_stripe/_droplet
 * uses a zero shift (:690, :739), the one left by bflbm_init_mixture the absolute COM (:623-625),
 * uploaded states (LBM_init) and every later step COM - com_ref (:651-654, :588).
 * bflbm_set_ref_state: per-box upload of the three one-component fields; they cover the GLOBAL
 * lattice on every slab.  While active the two-pass schedule is used (the shift needs the densities
 * of the whole lattice before the collision) and a slab of a decomposed lattice must be given the
 * global COM of the resident state with bflbm_set_com before each step (the ring and the python slab
 * driver do that; a single slab reduces it itself). */
int bflbm_set_ref_state(bflbm_ctx* c, const double* rho_eq, const double* phi_eq, const double* rhot_eq, const bflbm_fab* box);
int bflbm_enable_ref_state(bflbm_ctx* c, int on, const double com_ref[3]);
int bflbm_ref_state_active(const bflbm_ctx* c, int* active);   /* on, kBT != 0 and no injected noise pending */
int bflbm_set_com(bflbm_ctx* c, const double com[3]);

int bflbm_sync(bflbm_ctx* c);

/* ---- Structure factors on the device (FHDeX StructFact as the reference drives it: pair list
 * main_run_job.cpp:301-310, FortStructure every out_SF_step steps :342-349, WritePlotFile :50-54).
 * S_ab(k) = < a^(k) conj(b^(k)) > / N with un-normalised transforms (hipFFT D2Z), averaged over the
 * accumulated frames.  var_a/var_b index hydrovs (VariableNames order) or, with lb_hydrovars != 0,
 * hydrovsbar (the shipped STRUCT_LB_HYDROVARS build, main_run_job.cpp:19, :344); scale may be NULL (1).
 * bflbm_sf_get returns the full fft-shifted spectrum (k = 0 at cell n/2) [npairs][nz][ny][nx]:
 * what 0 magnitude, 1 real, 2 imaginary part; zero_avg != 0 removes k = 0.  Needs the whole lattice in
 * one context (nranks == 1).  hipFFT is loaded at first use; without it these calls fail, nothing else.
 * The accumulator is a recorder that stepping never serves (every = 0): bflbm_destroy of its context detaches it.
 * Detached, bflbm_sf_nsamples, _reset and _destroy work, bflbm_sf_accumulate fails, and so does bflbm_sf_get, whose
 * expansion is written into the context's scratch buffer.  Creation and a frame inside an open step are refused. */
typedef struct bflbm_sf bflbm_sf;
int bflbm_sf_create(bflbm_ctx* c, int npairs, const int* var_a, const int* var_b, const double* scale, bflbm_sf** out);
int bflbm_sf_destroy(bflbm_sf* s);
int bflbm_sf_reset(bflbm_sf* s);
int bflbm_sf_accumulate(bflbm_sf* s, int lb_hydrovars, int reset);
int bflbm_sf_nsamples(const bflbm_sf* s, long long* n);
int bflbm_sf_get(bflbm_sf* s, int what, int zero_avg, double* dst);

/* The same accumulator for a lattice decomposed into the z-slabs of a bflbm_ring (any number of slabs, on one or
 * several GPUs): 2-D transforms of every slab's own planes, a transpose over the slabs, z transforms of row blocks,
 * pair products per slab; bflbm_ring_sf_get assembles and expands the mean on the host.  A frame is stream-ordered like
 * a sample of the ring's spectrum trace: events between the slabs' streams and no host synchronisation (hydrovs under
 * a reference state excepted: the global centre of mass is summed on the host first).  The transpose reads its sources
 * in place where every slab is on one device or peer-mapped and neither bflbm_ring_set_transport(1) nor
 * BFLBM_RING_COPY_FALLBACK=1 asks for copies, by strided (peer) copies otherwise; both move the same doubles.
 * bflbm_ring_sf_get, _reset and _destroy order themselves after the frames enqueued.
 * Same arguments, normalisation and output layout as bflbm_sf_*; a ring of one slab delegates to it.  bflbm_ring_destroy
 * detaches the accumulator as bflbm_destroy does a lone one; detached, bflbm_ring_sf_get still works: it reads only the
 * accumulators the handle owns. */
typedef struct bflbm_ring_sf bflbm_ring_sf;
int bflbm_ring_sf_create(bflbm_ring* r, int npairs, const int* var_a, const int* var_b, const double* scale, bflbm_ring_sf** out);
int bflbm_ring_sf_destroy(bflbm_ring_sf* s);
int bflbm_ring_sf_reset(bflbm_ring_sf* s);
int bflbm_ring_sf_accumulate(bflbm_ring_sf* s, int lb_hydrovars, int reset);
int bflbm_ring_sf_nsamples(const bflbm_ring_sf* s, long long* n);
int bflbm_ring_sf_get(bflbm_ring_sf* s, int what, int zero_avg, double* dst);

/* ---- Droplet observables reduced on the device (Droplet_Fluctuation.ipynb / Surface_Tension.ipynb
 * cell 3; the reference's C++ twins getCenterOfMass / fittingDropletCovariance / fittingDropletParams,
 * LBM_hydrovs.H:62-335, are off by default, main_run_job.cpp:111).
 * moments[0..9]  = sum over the slab's cells of rho * {1, x, y, z, xx, xy, xz, yy, yz, zz}, x,y,z = GLOBAL
 * cell indices; moments[10..19] = the same with trapezoid weights (the lattice's end planes count half in
 * each direction: Integration::trapezoid3DWeightTensor, the notebook's wt).  Centre of mass, covariance
 * and principal axes follow on the host from these 20 numbers (analysis.py: *_from_moments).
 * bflbm_fit_droplet: least-squares fit of rho(r) = hi - (hi-lo)/2 (1 + tanh((r-R)/W)), r = distance of the
 * cell centre (i+1/2)/n from r0 in the unit box (the notebook's model), by Levenberg-Marquardt on normal
 * equations reduced on the device; params = (hi, lo, R, W) start values in, solution out. */
int bflbm_droplet_moments(bflbm_ctx* c, double moments[20]);
int bflbm_ring_droplet_moments(bflbm_ring* r, double moments[20]);
int bflbm_fit_droplet(bflbm_ctx* c, const double r0[3], double params[4], int max_iter, double tol, double* cost, int* iterations);
int bflbm_ring_fit_droplet(bflbm_ring* r, const double r0[3], double params[4], int max_iter, double tol, double* cost, int* iterations);

/* The reference's own radius fit (fittingDropletParams, LBM_hydrovs.H:160-213; call site main_run_job.cpp:364-367, off by
 * default: `if_print_radius = false`, :111): a semi-implicit gradient flow of (W, R) in
 * rho ~ 1/2 (1 + tanh((R - |r - r0|) / sqrt(2W))), unit-box coordinates, r0 = centre of mass of rho; `nstep` flow steps
 * from (W0, R0), the result is the mean over the last `step_window` steps, retried from that mean with dt / 5 (at most
 * `max_retry` times) while (max - min) / mean over the window exceeds `undul_ratio` for either parameter.  The two lattice
 * integrals of every step are reduced on the device; the closed-form coefficients (externlib.H:199-371) on the host.
 * result = { W, R, undulation }.  Returns non-zero (message in bflbm_last_error) where the reference throws: undulation still
 * out of bounds after the retries; result is filled nevertheless.  opts == NULL: the reference's default arguments
 * (W0 0.02, R0 0.3, eta 0.2, dt 0.02, 400 steps, window 30, undulation 0.005); the driver passes
 * (window 20, undulation 0.01, 400 steps, W0 = kappa, R0 = radius).  No output of this fit is recorded in the reference:
 * parity unpinned. */
typedef struct {
  double W0, R0, eta_W, eta_R, dt, undul_ratio;
  int nstep, step_window, max_retry;
} bflbm_flowfit_opts;
void bflbm_flowfit_default_opts(bflbm_flowfit_opts* o);
int bflbm_fit_droplet_flow(bflbm_ctx* c, const bflbm_flowfit_opts* opts, double result[3], int* retries);
int bflbm_ring_fit_droplet_flow(bflbm_ring* r, const bflbm_flowfit_opts* opts, double result[3], int* retries);
/* Host only: the closed forms of one flow step at (W, R) -- out = { J_RR, J_WR, J_RW, J_WW, K_W, K_R, I_2, I_3, I_4 }
 * with I_n = int_{-c}^{inf} (x + c)^n sech^4(x) dx, c = R / sqrt(2W) (externlib.H:108-157, :199-253, :344-371). */
int bflbm_flowfit_coefficients(double W, double R, double eta_W, double eta_R, double dt, double C0, double out[9]);

/* hipEvent timing on the context's stream: start, run steps, stop -> milliseconds. */
int bflbm_timer_start(bflbm_ctx* c);
int bflbm_timer_stop(bflbm_ctx* c, float* ms);

/* Host-side evaluation of the project's counter-based Gaussian stream (the HIP
 * kernels use the same code): out36[0..32] = the 33 normals of the site and noise index (3 momentum
 * modes, 15 modes of f, 15 modes of g), out36[33..35] = 0. */
int bflbm_rng_site_normals(uint64_t seed, uint64_t site, uint32_t noise_index, double* out36);

/* Diagnostics: time `reps` launches of a streaming kernel over the slab (hipEvents), for
 * roofline calibration.  which: 0 = pull-copy (38 shifted reads + 38 writes per site),
 * 1 = density pass (38 reads + 2 writes), 2 = hipMemcpyAsync device-to-device of one buffer.
 * The resident state is not modified (scratch buffer is overwritten). */
int bflbm_debug_time_kernel(bflbm_ctx* c, int which, int reps, float* ms_per_launch);

/* Device bytes held by the context. */
/* Physical placement.  A context's step time sits on one of a few discrete levels up to 8 % apart that belong to the physical
 * pages behind its allocation.  bflbm_tune_placement times a few steps of the context's own step kernel on
 * an analytic state, allocates up to max_candidates - 1 further candidates while holding the best so far, and keeps the fastest;
 * the context is left as freshly created (no state resident).  bflbm_create calls it with 4 candidates (8 when the state is below
 * 24 GB) for slabs of at least 2^21 sites (BFLBM_PLACEMENT_CANDIDATES=1: never; max_candidates: 1 ... 8).  ms_per_step (nullable): time of every candidate tried; kept (nullable): its index. */
int bflbm_tune_placement(bflbm_ctx* c, int max_candidates, float* ms_per_step, int* kept);
int bflbm_placement_report(const bflbm_ctx* c, float ms_per_step[8], int* tried, int* kept);   /* what the last tuning measured (tried = 0: never tuned) */
int bflbm_debug_addresses(const bflbm_ctx* c, unsigned long long out[8]);   /* diagnostics: device addresses of the state A, B, rho, phi, scratch, frames x 2; component stride in doubles */
int bflbm_device_bytes(const bflbm_ctx* c, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* BFLBM_H_ */
