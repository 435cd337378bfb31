"""GPU: ensemble traces (Trace, bflbm_trace_*): per-replica droplet moments recorded on the device every k steps.

A record must equal, bit for bit, what bflbm_droplet_moments gives for the same state (threshold = -inf), whatever the
schedule, the number of replicas, or whether the lattice is a replica or a lone context; with a threshold it is compared
with numpy sums of the downloaded density under the a-priori bound of a re-ordered sum.  A trace changes nothing its
owner computes.  The shapes are the smallest at which the kernels take another path: a plane smaller than one block, a
padded pitch with several blocks per plane, unequal extents with a ragged last block, nx no multiple of the padding, and
a lattice the hand-over schedule takes.  One path these shapes do not reach: with more than 256 blocks per plane
(pitch * ny > 65536) the strided loop of k_trace_finish and k_plane_partials runs a second time.  Those widths (256, 257,
270 and 556 blocks per plane; lone, batch and ring traces) are in tests/test_gpu_wide_planes.py, against exact sums of a
field in which every block carries weight."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 8), (24, 24, 24), (20, 28, 24), (72, 12, 10), (64, 8, 16)]
HANDOVER_SHAPE = (64, 8, 16)
NREC = 12


def _droplet(pkg, n, schedule=None, kBT=0.0, radius=0.25, steps=2, **params):
    """A droplet as in tests/test_gpu_droplet.py (alpha0 = 2.5, radius 0.25) after a few steps."""
    p = dict(alpha0=2.5, kBT=kBT)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_droplet(radius)
    lbm.LBM_timestep(steps)
    return lbm


def _check_full_record(rec, n):
    assert np.array_equal(rec[..., 10], rec[..., 0])                    # threshold -inf: the mass twice
    assert np.all(rec[..., 11] == n[0] * n[1] * n[2])


# ---- 1. exact against the existing reduction ---------------------------------------------------------------------------
CASES = [(n, s, kBT) for n in SHAPES for s in ("two_pass", "fused") for kBT in (0.0, 1e-5)]
CASES += [(HANDOVER_SHAPE, "handover", kBT) for kBT in (0.0, 1e-5)]


@pytest.mark.parametrize("n,schedule,kBT", CASES)
def test_lone_trace_equals_droplet_moments(pkg, n, schedule, kBT):
    a = _droplet(pkg, n, schedule, kBT)
    b = _droplet(pkg, n, schedule, kBT)                                  # the twin without a trace
    if schedule == "handover":
        assert a.resolved_schedule() == "handover" and b.resolved_schedule() == "handover"
    tr = a.trace(every=1, capacity=4, threshold=-np.inf)
    tr.sample()
    want = [b.droplet_moments()[:10]]
    for _ in range(3):
        a.LBM_timestep(1)
        b.LBM_timestep(1)
        want.append(b.droplet_moments()[:10])
    assert tr.count == 4
    steps, rec = tr.read()
    assert steps.shape == (4, 1) and steps.dtype == np.int64 and rec.shape == (4, 1, NREC)
    assert steps[:, 0].tolist() == [2, 3, 4, 5]
    for k in range(4):
        assert np.array_equal(rec[k, 0, :10], want[k]), (k, rec[k, 0, :10] - want[k])
    _check_full_record(rec, n)
    assert np.array_equal(a.droplet_moments()[:10], want[-1])            # the owner's own reduction is undisturbed
    assert np.array_equal(tr.com()[-1, 0], want[-1][1:4] / want[-1][0])
    a.close()
    assert tr._h is None                                                 # closing the owner closed its dependent
    b.close()


# ---- 2. a batch records what lone lattices give -------------------------------------------------------------------------
REPLICAS = [dict(alpha0=2.5, kappa=4.0, seed=11), dict(alpha0=2.0, kappa=2.0, seed=12), dict(alpha0=1.5, kappa=1.0, seed=13),
            dict(alpha0=2.2, kappa=3.0, seed=14), dict(alpha0=1.0, kappa=0.5, seed=15)]
RADII = [0.25, 0.2, 0.3, 0.15, 0.35]


def _batch_and_lones(pkg, n, nrep, schedule, kBT=1e-5):
    params = [dict(p, kBT=kBT) for p in REPLICAS[:nrep]]
    batch = pkg.BatchLBM(n, params=params, schedule=schedule)
    lones = [pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule) for p in params]
    for lat, r in zip(batch.replicas + lones, RADII[:nrep] * 2):
        lat.LBM_init_droplet(r)
    return batch, lones


@pytest.mark.parametrize("n,nrep,schedule", [((24, 24, 24), 5, "two_pass"), ((24, 24, 24), 5, "fused"),
                                             ((20, 28, 24), 1, "two_pass"), ((20, 28, 24), 1, "fused"),
                                             ((20, 28, 24), 3, "two_pass"), ((20, 28, 24), 3, "fused")])
def test_batch_trace_equals_lone_lattices(pkg, n, nrep, schedule):
    batch, lones = _batch_and_lones(pkg, n, nrep, schedule)
    assert batch.resolved_schedule() == schedule
    tr = batch.trace(every=1, capacity=7, threshold=-np.inf)
    tr.sample()
    want = [[lone.droplet_moments()[:10] for lone in lones]]
    for _ in range(6):
        batch.LBM_timestep(1)
        for lone in lones:
            lone.LBM_timestep(1)
        want.append([lone.droplet_moments()[:10] for lone in lones])
    steps, rec = tr.read()
    assert rec.shape == (7, nrep, NREC)
    assert np.array_equal(steps, np.arange(7)[:, None] * np.ones((1, nrep), dtype=np.int64))
    assert np.array_equal(rec[..., :10], np.array(want))
    _check_full_record(rec, n)
    batch.close()
    for lone in lones:
        lone.close()


def test_batch_trace_every_third_step(pkg):
    n, nrep = (24, 24, 24), 3
    batch, lones = _batch_and_lones(pkg, n, nrep, "two_pass")
    tr = batch.trace(every=3, capacity=4, threshold=-np.inf)
    want = {}
    batch.LBM_timestep(4)                                                # one call spanning a sample, then single steps
    for s in range(1, 8):
        for lone in lones:
            lone.LBM_timestep(1)
        want[s] = np.array([lone.droplet_moments()[:10] for lone in lones])
    batch.LBM_timestep(3)
    assert tr.count == 2
    steps, rec = tr.read()
    assert steps.tolist() == [[3] * nrep, [6] * nrep]
    assert np.array_equal(rec[0, :, :10], want[3]) and np.array_equal(rec[1, :, :10], want[6])
    batch.close()
    for lone in lones:
        lone.close()


# ---- 3. threshold --------------------------------------------------------------------------------------------------------
# LBM_init_droplet centres the droplet at z = nx / 2 (LBM_binary.H:725 measures z with box[0]): in the flat 72 x 12 x 10 box a
# droplet of radius 0.25 nx lies wholly outside the lattice and no cell reaches 0.06; radius 0.4 nx puts its cap inside.
@pytest.mark.parametrize("n,radius", [((24, 24, 24), 0.25), ((72, 12, 10), 0.4)])
def test_threshold_against_numpy(pkg, n, radius):
    thr = 0.06
    lbm = _droplet(pkg, n, radius=radius, steps=4)
    tr = lbm.trace(every=1, capacity=1, threshold=thr)
    tr.sample()
    rec = tr.read()[1][0, 0]
    rho = lbm.LBM_hydrovars_density(ncomp=1)[0]                          # (nz, ny, nx): the doubles the kernel compares
    nsites = rho.size
    mask = rho > thr
    assert 0 < mask.sum() < nsites                                       # the threshold is doing something
    assert rec[11] == mask.sum()
    z, y, x = [v.astype(np.float64) for v in np.meshgrid(*[np.arange(k) for k in rho.shape], indexing="ij")]
    weights = [np.ones_like(rho), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    eps = 2.0 ** -53
    for k, w in enumerate(weights):
        terms = np.where(mask, rho * w, 0.0)                             # the same rounded products the kernel adds
        # a-priori bound of any summation order of the same terms; the factor 2 covers numpy's own sum
        bound = 2 * nsites * eps * np.abs(terms).sum()
        err = abs(rec[k] - terms.sum())
        print(f"{n} moment {k}: |trace - numpy| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    err, bound = abs(rec[10] - rho.sum()), 2 * nsites * eps * np.abs(rho).sum()
    print(f"{n} mass: |trace - numpy| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    lbm.close()


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------
def test_trace_changes_nothing_the_owner_computes(pkg):
    n = (24, 24, 24)
    a, b = _droplet(pkg, n, kBT=1e-5, steps=0), _droplet(pkg, n, kBT=1e-5, steps=0)
    ta = a.trace(every=1, capacity=8, threshold=0.06)
    ta.sample()
    a.LBM_timestep(2); b.LBM_timestep(2)
    a.LBM_timestep(3); b.LBM_timestep(3)
    assert ta.count == 6 and a.steps_done == b.steps_done == 5
    for u, v in zip(a.populations() + (a.LBM_hydrovars(),), b.populations() + (b.LBM_hydrovars(),)):
        assert np.array_equal(u, v)
    a.close(); b.close()

    (ba, la), (bb, lb) = _batch_and_lones(pkg, n, 3, None), _batch_and_lones(pkg, n, 3, None)
    tb = ba.trace(every=1, capacity=8)
    tb.sample()
    ba.LBM_timestep(5); bb.LBM_timestep(5)
    assert tb.count == 6
    assert [r.steps_done for r in ba.replicas] == [r.steps_done for r in bb.replicas] == [5, 5, 5]
    for u, v in zip(ba.populations() + (ba.LBM_hydrovars(),), bb.populations() + (bb.LBM_hydrovars(),)):
        assert np.array_equal(u, v)
    for lat in [ba, bb] + la + lb:
        lat.close()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------
# every = 2, capacity = 3.  By the sampling rule a call of 7 steps from a fresh trace adds the samples of steps 2, 4 and 6,
# which fit; the first call that does not fit is 8 steps (or 7 steps once one step has been taken).  Both are asserted.
def _capacity_protocol(pkg, owner, steps_done):
    tr = owner.trace(every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="trace full"):
        owner.LBM_timestep(8)                                            # samples at 2, 4, 6, 8
    assert steps_done() == 0 and tr.count == 0
    for _ in range(2):
        owner.LBM_timestep(6)
        assert tr.count == 3
        with pytest.raises(pkg.BflbmError, match="trace full"):
            tr.sample()
        assert tr.count == 3
        tr.reset()
        assert tr.count == 0
    owner.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="trace full"):
        owner.LBM_timestep(7)                                            # one step in: samples at 2, 4, 6, 8
    assert steps_done() == 13 and tr.count == 0
    owner.LBM_timestep(6)                                                # ... and 6 more fill it exactly
    assert steps_done() == 19 and tr.count == 3
    return tr


def test_capacity_lone(pkg):
    lbm = _droplet(pkg, (24, 24, 24), steps=0)
    tr = _capacity_protocol(pkg, lbm, lambda: lbm.steps_done)            # leaves the trace full, 7 steps since its reset
    state = lbm.populations()
    with pytest.raises(pkg.BflbmError, match="trace full"):
        lbm.step_boundary()                                              # the eighth step would sample
    with pytest.raises(pkg.BflbmError, match="bflbm_step_boundary first"):
        lbm.step_interior()                                              # the refused step is not open
    assert lbm.steps_done == 19 and tr.count == 3
    assert all(np.array_equal(u, v) for u, v in zip(state, lbm.populations()))
    lbm.close()


def test_capacity_batch(pkg):
    batch, lones = _batch_and_lones(pkg, (24, 24, 24), 3, None, kBT=0.0)
    _capacity_protocol(pkg, batch, lambda: max(r.steps_done for r in batch.replicas))
    assert [r.steps_done for r in batch.replicas] == [19, 19, 19]
    for lat in [batch] + lones:
        lat.close()


# ---- 6. labels --------------------------------------------------------------------------------------------------------------
def test_labels_follow_each_replicas_step_counter(pkg):
    batch, lones = _batch_and_lones(pkg, (8, 8, 8), 3, None)
    batch.replicas[1].set_steps_done(1000)
    tr = batch.trace(every=1, capacity=4)
    tr.sample()
    batch.LBM_timestep(3)
    steps, _ = tr.read()
    assert steps[:, 1].tolist() == [1000, 1001, 1002, 1003]
    assert steps[:, 0].tolist() == steps[:, 2].tolist() == [0, 1, 2, 3]
    for lat in [batch] + lones:
        lat.close()


# ---- 7. refusals and lifetime ----------------------------------------------------------------------------------------------
def test_creation_refusals(pkg):
    lib = pkg._lib.load()

    def refused(create, handle, every, capacity, threshold, pattern):
        h = ctypes.c_void_p()
        rc = getattr(lib, create)(handle, every, capacity, threshold, ctypes.byref(h))
        msg = lib.bflbm_last_error().decode()
        assert rc != 0 and not h.value, (create, pattern)
        assert pattern in msg, msg

    lbm = _droplet(pkg, (8, 8, 8), steps=0)
    batch, lones = _batch_and_lones(pkg, (8, 8, 8), 2, None)
    for create, owner in (("bflbm_trace_create", lbm), ("bflbm_batch_trace_create", batch)):
        refused(create, owner._h, 0, 4, 0.0, "every")
        refused(create, owner._h, -2, 4, 0.0, "every")
        refused(create, owner._h, 1, 0, 0.0, "capacity")
        refused(create, owner._h, 1, 4, float("nan"), "NaN")
    refused("bflbm_trace_create", batch.replicas[0]._h, 1, 4, 0.0, "bflbm_batch_trace_create")
    with pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2) as slab:
        refused("bflbm_trace_create", slab._h, 1, 4, 0.0, "nranks > 1")
    for owner, create in ((lbm, "bflbm_trace_create"), (batch, "bflbm_batch_trace_create")):
        tr = owner.trace(1, 4)
        refused(create, owner._h, 1, 4, 0.0, "already has a trace")
        with pytest.raises(pkg.BflbmError, match="already has a trace"):
            owner.trace(1, 4)
        tr.close()
        owner.trace(1, 4).close()                                        # a closed trace makes room for the next
    # an open step refuses creation, and sample / reset / read of an existing trace
    lbm.step_boundary()
    refused("bflbm_trace_create", lbm._h, 1, 4, 0.0, "open step")
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.trace(1, 4)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.reset, tr.read):
        with pytest.raises(pkg.BflbmError, match="open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2
    for lat in [lbm, batch] + lones:
        lat.close()


def test_trace_outlives_its_owner(pkg):
    """Through the raw ABI: destroying the owner detaches the trace; its samples stay readable."""
    lib = pkg._lib.load()
    check = pkg._lib.check
    p = pkg.default_params(alpha0=2.5)
    d = pkg.Domain()
    d.n[0], d.n[1], d.n[2] = 24, 24, 24
    d.z0, d.z1, d.rank, d.nranks, d.device = 0, 24, 0, 1, 0
    c, t = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bflbm_create(ctypes.byref(p), ctypes.byref(d), ctypes.byref(c)))
    check(lib.bflbm_init_droplet(c, 0.25))
    check(lib.bflbm_trace_create(c, 1, 8, -np.inf, ctypes.byref(t)))
    check(lib.bflbm_trace_sample(t))
    check(lib.bflbm_step(c, 2))

    def read():
        n, b = ctypes.c_longlong(), ctypes.c_int()
        check(lib.bflbm_trace_count(t, ctypes.byref(n), ctypes.byref(b)))
        rec = np.empty((n.value, b.value, NREC))
        steps = np.empty((n.value, b.value), dtype=np.int64)
        check(lib.bflbm_trace_read(t, 0, n.value, rec.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.c_void_p)))
        return steps, rec

    steps0, rec0 = read()
    assert steps0[:, 0].tolist() == [0, 1, 2]
    check(lib.bflbm_destroy(c))
    steps1, rec1 = read()
    assert np.array_equal(steps0, steps1) and np.array_equal(rec0, rec1)
    assert lib.bflbm_trace_sample(t) != 0
    assert "destroyed" in lib.bflbm_last_error().decode()
    tail = np.empty((1, 1, NREC))
    check(lib.bflbm_trace_read(t, 2, 1, tail.ctypes.data_as(ctypes.c_void_p), None))     # a window, without labels
    assert np.array_equal(tail[0], rec0[2])
    assert lib.bflbm_trace_read(t, 2, 2, tail.ctypes.data_as(ctypes.c_void_p), None) != 0
    check(lib.bflbm_trace_destroy(t))


# ---- 8. split step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,schedule", [((24, 24, 24), "two_pass"), (HANDOVER_SHAPE, "handover")])
def test_split_step_samples_like_a_whole_step(pkg, n, schedule):
    a, b = _droplet(pkg, n, schedule, kBT=1e-5), _droplet(pkg, n, schedule, kBT=1e-5)
    ta, tb = a.trace(1, 2), b.trace(1, 2)
    a.step_boundary(); a.step_interior()
    assert ta.count == 0
    a.step_finish()
    b.LBM_timestep(1)
    assert ta.count == tb.count == 1
    (sa, ra), (sb, rb) = ta.read(), tb.read()
    assert sa.tolist() == sb.tolist() == [[3]]
    assert np.array_equal(ra, rb)
    assert np.array_equal(ra[0, 0, :10], b.droplet_moments()[:10])
    a.close(); b.close()
