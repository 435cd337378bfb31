"""GPU: shape traces (ShapeTrace, bflbm_shape_*): the radius at which a density contour of a droplet is met along fixed
rays from a centre, for every replica, found on the device every k steps.

The definition is in include/bflbm.h ("Shape traces"); analysis.droplet_radii restates it in numpy.  A sample must equal
that restatement applied to the downloaded density of the same state at the recorded centre: the same arithmetic on the
same doubles, so every comparison is exact, with NaNs (rays without a crossing) matched by position.  The centre of mass
must equal records 1-3 / record 0 of an ensemble trace with the same threshold, exactly.  A trace changes nothing its owner
computes.  The shapes, the droplet helper and the radii are those of tests/test_gpu_iface.py."""
import ctypes

import numpy as np
import pytest

from observable_twins import same_doubles as _same

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 8), (24, 24, 24), (20, 28, 24), (72, 12, 10), (64, 8, 16)]
HANDOVER_SHAPE = (64, 8, 16)
# LBM_init_droplet centres the droplet at z = nx / 2 with radius r nx (LBM_binary.H:725): in the two flat boxes the droplet's
# cap lies inside the lattice, a slab through all of y.  On (64, 8, 16) the rho = 0.5 surface is 4.5 ... 12.7 cells from the
# centre of mass along the 32 rays of ray_nodes(4, 8) (phi = 0.5: up to 17 cells from the fixed centre), so that box needs
# rays longer than half its smallest extent (they wrap).  On (72, 12, 10) the cap is thin and decays (the CPU oracle gives
# max rho 0.73 after 2 steps and 0.59 after 5), so its levels are rho = 0.2 (radii 1.0 ... 11.1) and phi = 0.8 (2.5 ... 7.5).
# With these settings the CPU oracle finds a crossing on every ray after 2 to 5 steps at kBT = 0 and 1e-5 on every shape;
# each test asserts on what it compares that the radii are finite and not all equal.
RADIUS = {(8, 8, 8): 0.25, (24, 24, 24): 0.25, (20, 28, 24): 0.25, (72, 12, 10): 0.4, (64, 8, 16): 0.4}
RMAX = {(72, 12, 10): 16.0, (64, 8, 16): 20.0}
LEVELS = {(72, 12, 10): (0.2, 0.8)}                                      # (rho, phi); elsewhere (rho_hi + rho_lo) / 2 for both
# a fixed centre near the centre of mass of the initial profile, on no lattice site
FIXED = {(8, 8, 8): (4.3, 3.8, 4.1), (24, 24, 24): (12.3, 11.8, 12.1), (20, 28, 24): (10.3, 13.8, 10.1),
         (72, 12, 10): (36.3, 5.8, 8.1), (64, 8, 16): (32.3, 3.8, 12.1)}
THRESHOLD = 0.06
W = np.array([1 / 3] + [1 / 18] * 6 + [1 / 36] * 12)[:, None, None, None]


def _droplet(pkg, n, schedule=None, kBT=0.0, radius=None, steps=2, **params):
    """A droplet as in tests/test_gpu_trace.py (alpha0 = 2.5) after a few steps."""
    p = dict(alpha0=2.5, kBT=kBT)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_droplet(RADIUS[n] if radius is None else radius)
    lbm.LBM_timestep(steps)
    return lbm


def _levels(lbm, n):
    mid = (lbm.params.rho_hi + lbm.params.rho_lo) / 2
    return LEVELS.get(n, (mid, mid))


def _densities(lbm):
    """rho, phi [nz, ny, nx] of the resident state: the doubles the kernel forms."""
    return lbm.LBM_hydrovars_density(ncomp=2)


def _nodes(pkg):
    return pkg.analysis.ray_nodes(4, 8)


def _nsteps(n, step=0.5, rmax=None):
    return int(np.floor((min(n) / 2 if rmax is None else rmax) / step))


def _finite_and_varied(r):
    return bool(np.isfinite(r).all()) and np.unique(r).size > 1


# ---- 1. a lone droplet: every sample equals the restatement on a twin without a trace ------------------------------------
CASES = [(n, s, kBT) for n in SHAPES for s in ("two_pass", "fused") for kBT in (0.0, 1e-5)]
CASES += [(HANDOVER_SHAPE, "handover", kBT) for kBT in (0.0, 1e-5)]


@pytest.mark.parametrize("n,schedule,kBT", CASES)
def test_lone_shape_trace_equals_the_restatement(pkg, n, schedule, kBT):
    a = _droplet(pkg, n, schedule, kBT)
    b = _droplet(pkg, n, schedule, kBT)                                  # the twin without a shape trace
    if schedule == "handover":
        assert a.resolved_schedule() == "handover" and b.resolved_schedule() == "handover"
    (level, level_phi), nodes, rmax = _levels(a, n), _nodes(pkg), RMAX.get(n)
    dirs = nodes[0]
    nsteps = _nsteps(n, rmax=rmax)
    assert np.array_equal(a.droplet_moments(), b.droplet_moments())
    t_rho = a.shape_trace(level, nodes, field="rho", direction="falling", threshold=THRESHOLD, rmax=rmax, every=1, capacity=4)
    t_phi = a.shape_trace(level_phi, nodes, field="phi", direction="rising", centre=FIXED[n], rmax=rmax, every=1, capacity=4)
    moments = b.trace(every=1, capacity=4, threshold=THRESHOLD)
    for tr in (t_rho, t_phi, moments):
        tr.sample()
    fields = [_densities(b)]
    for _ in range(3):
        a.LBM_timestep(1)
        b.LBM_timestep(1)
        fields.append(_densities(b))
    rec = moments.read()[1]
    com = rec[:, 0, 1:4] / rec[:, 0, 0:1]
    for tr in (t_rho, t_phi):
        assert tr.count == 4 and tr.geometry()[:2] == (len(dirs), nsteps)
    steps, centre, r = t_rho.read()
    assert steps.shape == (4, 1) and steps.dtype == np.int64 and centre.shape == (4, 1, 3) and r.shape == (4, 1, len(dirs))
    assert steps[:, 0].tolist() == [2, 3, 4, 5]
    assert np.array_equal(centre[:, 0], com) and np.array_equal(moments.com()[:, 0], com)      # Trace.com() bit for bit
    for s in range(4):
        want = pkg.analysis.droplet_radii(fields[s][0], centre[s, 0], dirs, level, 0.5, nsteps, "falling")
        assert _finite_and_varied(want), ("rho", s, want)                # the comparison below is about something
        assert _same(r[s, 0], want), ("rho", s)
    steps, centre, r = t_phi.read()
    assert steps[:, 0].tolist() == [2, 3, 4, 5]
    assert np.array_equal(centre[:, 0], np.tile(np.array(FIXED[n]), (4, 1)))
    for s in range(4):
        want = pkg.analysis.droplet_radii(fields[s][1], FIXED[n], dirs, level_phi, 0.5, nsteps, "rising")
        assert _finite_and_varied(want), ("phi", s, want)
        assert _same(r[s, 0], want), ("phi", s)
    modes = t_rho.modes(2)
    assert modes.shape == (4, 1, 9) and _same(modes, pkg.analysis.shape_modes(t_rho.read()[2], dirs, nodes[1], 2))
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.droplet_moments(), b.droplet_moments())      # the owner's own reduction is undisturbed
    a.close()
    assert t_rho._h is None and t_phi._h is None                         # closing the owner closed its dependents
    b.close()


# ---- 2. segments ---------------------------------------------------------------------------------------------------------
def test_segments_change_nothing(pkg):
    """One segment, several segments, a ragged last segment, both NaN and finite radii in one sample, and a crossing on the
    first pair of a later segment (its inner point is the last point of the segment before)."""
    nodes = _nodes(pkg)
    dirs = nodes[0]
    seen, mixed = [], False
    for n, step, rmax in [((24, 24, 24), 1.0, 7.0), ((24, 24, 24), 0.5, 12.0), ((24, 24, 24), 0.5, 6.5), ((24, 24, 24), 0.25, 12.0),
                          ((72, 12, 10), 0.5, 4.0), ((72, 12, 10), 0.3, 5.0), ((72, 12, 10), 0.5, 11.0)]:
        lbm = _droplet(pkg, n, kBT=1e-5, steps=3)
        level, level_phi = _levels(lbm, n)
        nsteps = _nsteps(n, step, rmax)
        t_rho = lbm.shape_trace(level, nodes, threshold=THRESHOLD, step=step, rmax=rmax, capacity=1)
        t_phi = lbm.shape_trace(level_phi, nodes, field="phi", direction="rising", centre=FIXED[n], step=step, rmax=rmax, capacity=1)
        ndir, k, nseg, seg_len = t_rho.geometry()
        assert (ndir, k) == (len(dirs), nsteps) and t_phi.geometry() == t_rho.geometry()
        assert nseg >= 1 and (nseg - 1) * seg_len < nsteps <= nseg * seg_len     # the segments cover the pairs, none is empty
        assert nseg == 1 or seg_len >= 4
        seen.append((nseg, nsteps % seg_len != 0))
        rho, phi = _densities(lbm)
        t_rho.sample(); t_phi.sample()
        _, centre, r = t_rho.read()
        want = pkg.analysis.droplet_radii(rho, centre[0, 0], dirs, level, step, nsteps)
        assert np.isfinite(want).any() and _same(r[0, 0], want), (n, step, rmax)
        if n == (72, 12, 10) and rmax == 4.0:                            # between the smallest (1.4) and the largest (9.6) radius of this state
            assert np.isnan(want).any() and np.isfinite(want).any(), want
            mixed = True
        want = pkg.analysis.droplet_radii(phi, FIXED[n], dirs, level_phi, step, nsteps, "rising")
        assert np.isfinite(want).any() and _same(t_phi.read()[2][0, 0], want), (n, step, rmax)
        lbm.close()
    assert mixed
    assert any(s == 1 for s, _ in seen) and any(s > 1 for s, _ in seen) and any(s > 1 and ragged for s, ragged in seen), seen

    # a crossing on the pair that straddles two segments: a radial step profile whose radius lies just beyond the last
    # point of segment 1, uploaded as f_i = w_i rho
    n, step, rmax = (24, 24, 24), 0.5, 12.0
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5))
    probe = lbm.shape_trace(0.5, nodes, centre=FIXED[n], step=step, rmax=rmax, capacity=1)
    _, nsteps, nseg, seg_len = probe.geometry()
    probe.close()
    assert nseg > 2
    z, y, x = np.meshgrid(*[np.arange(m) - 12.0 for m in (n[2], n[1], n[0])], indexing="ij")
    profile = np.where(np.sqrt(x * x + y * y + z * z) < (2 * seg_len + 0.6) * step, 0.9, 0.1)
    f0 = np.ascontiguousarray(W * profile[None])
    g0 = np.ascontiguousarray(W * (1.0 - profile)[None])
    lbm.LBM_init(f0, g0)
    tr = lbm.shape_trace(0.5, nodes, centre=FIXED[n], step=step, rmax=rmax, capacity=1)
    assert tr.geometry() == (len(dirs), nsteps, nseg, seg_len)
    tr.sample()
    want = pkg.analysis.droplet_radii(_densities(lbm)[0], FIXED[n], dirs, 0.5, step, nsteps)
    pair = np.floor(want / step)                                         # k - 1 of the pair a ray crosses on
    assert _finite_and_varied(want) and ((pair >= seg_len) & (pair % seg_len == 0)).any(), want
    assert _same(tr.read()[2][0, 0], want)
    lbm.close()


# ---- 3. a batch records what lone lattices give ---------------------------------------------------------------------------
REPLICAS = [dict(alpha0=2.5, kappa=4.0, seed=11), dict(alpha0=2.0, kappa=2.0, seed=12), dict(alpha0=1.5, kappa=1.0, seed=13)]
RADII = [0.25, 0.2, 0.0]              # radius 0: the profile peaks at 0.5, so nothing of replica 2 is above 0.7
AHEAD = 7                             # replica 1 joins with its step counter ahead: its noise and its labels follow it


def _batch_and_lones(pkg, n, schedule, kBT=1e-5):
    batch = pkg.BatchLBM(n, params=[dict(p, kBT=kBT) for p in REPLICAS], schedule=schedule)
    lones = [pkg.BinaryLBM(*n, params=pkg.default_params(**dict(p, kBT=kBT)), schedule=schedule) for p in REPLICAS]
    for owner in (batch.replicas, lones):
        for lat, r in zip(owner, RADII):
            lat.LBM_init_droplet(r)
        owner[1].set_steps_done(AHEAD)
    return batch, lones


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_batch_shape_trace_equals_lone_lattices(pkg, schedule):
    n, level = (24, 24, 24), 0.5
    nodes = _nodes(pkg)
    batch, lones = _batch_and_lones(pkg, n, schedule)
    assert batch.resolved_schedule() == schedule

    def make(owner):
        return [owner.shape_trace(level, nodes, threshold=THRESHOLD, every=1, capacity=4),
                owner.shape_trace(level, nodes, threshold=0.7, every=1, capacity=4),
                owner.shape_trace(level, nodes, field="phi", direction="rising", centre=FIXED[n], every=2, capacity=2)]

    traces = make(batch)
    lone_traces = [make(lone) for lone in lones]
    for tr in traces[:2] + [t for ts in lone_traces for t in ts[:2]]:
        tr.sample()
    batch.LBM_timestep(3)
    for lone in lones:
        lone.LBM_timestep(3)
    for k, tr in enumerate(traces):
        steps, centre, r = tr.read()
        count = (4, 4, 1)[k]
        assert steps.shape == (count, 3) and centre.shape == (count, 3, 3) and r.shape == (count, 3, len(nodes[0]))
        for rep in range(3):
            ls, lc, lr = lone_traces[rep][k].read()
            assert np.array_equal(steps[:, rep], ls[:, 0]), (k, rep)
            assert _same(centre[:, rep], lc[:, 0]) and _same(r[:, rep], lr[:, 0]), (k, rep)
        if k < 2:
            assert steps.tolist() == [[s, AHEAD + s, s] for s in range(4)]
        else:
            assert steps.tolist() == [[2, AHEAD + 2, 2]]
        for rep in (0, 1):
            assert all(_finite_and_varied(r[s, rep]) for s in range(count)), (k, rep)
        if k == 1:                                                       # nothing of replica 2 is above the threshold
            assert np.isnan(centre[:, 2]).all() and np.isnan(r[:, 2]).all()
            assert np.isfinite(centre[:, :2]).all()
    rho2 = _densities(lones[2])[0]
    assert rho2.max() < 0.7
    for lat in [batch] + lones:
        lat.close()
    assert all(tr._h is None for tr in traces)


# ---- 4. rules ---------------------------------------------------------------------------------------------------------------
# every = 2, capacity = 3 (the protocol of tests/test_gpu_iface.py): 7 steps from a fresh trace add the samples of steps 2, 4
# and 6, which fit; 8 steps do not.
def _overflow_protocol(pkg, owner, steps_done):
    nodes = _nodes(pkg)
    first = owner.shape_trace(0.5, nodes, every=1, capacity=64)          # served first; must not be touched by a refusal
    tr = owner.shape_trace(0.5, nodes, field="phi", direction="rising", centre=(12.3, 11.8, 12.1), every=2, capacity=3)
    state = owner.populations()
    with pytest.raises(pkg.BflbmError, match="shape trace full"):
        owner.LBM_timestep(8)                                            # samples at 2, 4, 6, 8
    assert steps_done() == 0 and tr.count == 0 and first.count == 0
    assert all(np.array_equal(u, v) for u, v in zip(state, owner.populations()))
    owner.LBM_timestep(6)
    assert tr.count == 3 and first.count == 6
    with pytest.raises(pkg.BflbmError, match="shape trace full"):
        tr.sample()
    assert tr.count == 3
    tr.reset()                                                           # reset restarts the count of steps as well
    assert tr.count == 0 and first.count == 6
    owner.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="shape trace full"):
        owner.LBM_timestep(7)                                            # one step in: samples at 2, 4, 6, 8
    assert steps_done() == 7 and tr.count == 0 and first.count == 7
    owner.LBM_timestep(6)
    assert steps_done() == 13 and tr.count == 3
    assert tr.read()[0][:, 0].tolist() == [8, 10, 12]                    # since the reset: steps 2, 4, 6 of 7
    return tr


def test_overflow_is_refused_before_any_launch_lone(pkg):
    lbm = _droplet(pkg, (24, 24, 24), steps=0)
    tr = _overflow_protocol(pkg, lbm, lambda: lbm.steps_done)            # leaves the trace full, 7 steps since its reset
    state = lbm.populations()
    with pytest.raises(pkg.BflbmError, match="shape trace full"):
        lbm.step_boundary()                                              # the eighth step would sample
    with pytest.raises(pkg.BflbmError, match="bflbm_step_boundary first"):
        lbm.step_interior()                                              # the refused step is not open
    assert lbm.steps_done == 13 and tr.count == 3
    assert all(np.array_equal(u, v) for u, v in zip(state, lbm.populations()))
    lbm.close()


def test_overflow_is_refused_before_any_launch_batch(pkg):
    batch = pkg.BatchLBM((24, 24, 24), params=[dict(p, kBT=0.0) for p in REPLICAS])
    for lat, r in zip(batch.replicas, RADII):
        lat.LBM_init_droplet(r)
    _overflow_protocol(pkg, batch, lambda: max(r.steps_done for r in batch.replicas))
    assert [r.steps_done for r in batch.replicas] == [13, 13, 13]
    batch.close()


def test_creation_refusals(pkg):
    lib = pkg._lib.load()
    nan, inf = float("nan"), float("inf")
    unit = [0.0, 0.0, 1.0, 0.6, 0.0, 0.8]

    def refused(create, handle, pattern, field=0, level=0.5, direction=0, centre=None, threshold=0.06, ndir=2, dirs=unit,
                step=0.5, nsteps=8, every=1, capacity=4):
        h = ctypes.c_void_p()
        c = None if centre is None else (ctypes.c_double * 3)(*centre)
        u = None if dirs is None else (ctypes.c_double * len(dirs))(*dirs)
        rc = getattr(lib, create)(handle, field, level, direction, c, threshold, ndir, u, step, nsteps, every, capacity, ctypes.byref(h))
        msg = lib.bflbm_last_error().decode()
        assert rc != 0 and not h.value, (create, pattern)
        assert pattern in msg and create in msg, msg

    lbm = _droplet(pkg, (8, 8, 8), steps=0)
    batch = pkg.BatchLBM((8, 8, 8), params=[dict(p) for p in REPLICAS[:2]])
    for lat in batch.replicas:
        lat.LBM_init_droplet(0.25)
    u2 = (ctypes.c_double * 6)(*unit)
    for create, owner in (("bflbm_shape_create", lbm), ("bflbm_batch_shape_create", batch)):
        assert getattr(lib, create)(owner._h, 0, 0.5, 0, None, 0.06, 2, u2, 0.5, 8, 1, 4, None) != 0   # no place for the handle
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and create in msg, msg
        refused(create, owner._h, "null", dirs=None)
        refused(create, owner._h, "field", field=2)
        refused(create, owner._h, "field", field=-1)
        refused(create, owner._h, "direction must", direction=2)
        refused(create, owner._h, "direction must", direction=-1)
        refused(create, owner._h, "level is NaN", level=nan)
        refused(create, owner._h, "threshold is NaN", threshold=nan)
        refused(create, owner._h, "centre", centre=(1.0, nan, 1.0))
        refused(create, owner._h, "centre", centre=(inf, 1.0, 1.0))
        refused(create, owner._h, "ndir", ndir=0)
        refused(create, owner._h, "ndir", ndir=65537)
        refused(create, owner._h, "direction 1", dirs=[0.0, 0.0, 1.0, 0.6, nan, 0.8])
        refused(create, owner._h, "direction 1", dirs=[0.0, 0.0, 1.0, 0.6, inf, 0.8])
        refused(create, owner._h, "direction 0", dirs=[0.0, 0.0, 1.00001, 0.6, 0.0, 0.8])
        refused(create, owner._h, "direction 1", dirs=[0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
        refused(create, owner._h, "step", step=0.0)
        refused(create, owner._h, "step", step=-0.5)
        refused(create, owner._h, "step", step=nan)
        refused(create, owner._h, "step", step=inf)
        refused(create, owner._h, "nsteps", nsteps=0)
        refused(create, owner._h, "every", every=0)
        refused(create, owner._h, "capacity", capacity=0)
        refused(create, owner._h, "1 TB", capacity=1 << 40)
        # what is accepted at the edges: a NaN threshold beside a fixed centre, a direction within 1e-6 of unit length
        h = ctypes.c_void_p()
        c = (ctypes.c_double * 3)(4.0, 4.0, 4.0)
        ok = (ctypes.c_double * 6)(0.0, 0.0, 1.0 + 4e-7, 0.6, 0.0, 0.8)
        pkg._lib.check(getattr(lib, create)(owner._h, 0, 0.5, 0, c, nan, 2, ok, 0.5, 8, 1, 4, ctypes.byref(h)))
        pkg._lib.check(lib.bflbm_shape_destroy(h))
    refused("bflbm_shape_create", batch.replicas[0]._h, "bflbm_batch_shape_create")
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_shape_create"):
        batch.replicas[0].shape_trace(0.5)
    with pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2) as slab:
        refused("bflbm_shape_create", slab._h, "nranks > 1")
    with pytest.raises(ValueError):
        lbm.shape_trace(0.5, field="density")
    with pytest.raises(ValueError):
        lbm.shape_trace(0.5, direction="sideways")
    with pytest.raises(ValueError):
        lbm.shape_trace(0.5, nodes=(np.zeros((4, 2)), np.zeros(4)))
    # an open step refuses creation, and sample / reset / read of an existing trace
    tr = lbm.shape_trace(0.5, _nodes(pkg), capacity=4)
    assert tr.geometry()[:2] == (32, 8)                                  # the defaults: step 0.5 out to min(n) / 2
    tr.sample()
    lbm.step_boundary()
    refused("bflbm_shape_create", lbm._h, "open step")
    for call in (tr.sample, tr.reset, tr.read):
        with pytest.raises(pkg.BflbmError, match="open step"):
            call()
    assert tr.count == 1
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2                                                 # the split step samples in its finish
    assert tr.read()[0][:, 0].tolist() == [0, 1]
    tr.reset()
    assert tr.count == 0 and tr.read()[2].shape == (0, 1, 32)
    default = lbm.shape_trace(0.5, capacity=1)                           # nodes default to ray_nodes(16, 32)
    assert default.geometry()[:2] == (512, 8) and np.array_equal(default.dirs, pkg.analysis.ray_nodes(16, 32)[0])
    for lat in (lbm, batch):
        lat.close()


def test_shape_trace_outlives_its_owner(pkg):
    """Through the raw ABI: destroying the owner detaches the trace; its samples stay readable."""
    lib = pkg._lib.load()
    check = pkg._lib.check
    p = pkg.default_params(alpha0=2.5)
    d = pkg.Domain()
    d.n[0], d.n[1], d.n[2] = 24, 24, 24
    d.z0, d.z1, d.rank, d.nranks, d.device = 0, 24, 0, 1, 0
    dirs = np.ascontiguousarray(_nodes(pkg)[0])
    c, t = ctypes.c_void_p(), ctypes.c_void_p()
    check(lib.bflbm_create(ctypes.byref(p), ctypes.byref(d), ctypes.byref(c)))
    check(lib.bflbm_init_droplet(c, 0.25))
    check(lib.bflbm_shape_create(c, 0, 0.5, 0, None, 0.06, len(dirs), dirs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 0.5, 24, 1, 8, ctypes.byref(t)))
    check(lib.bflbm_shape_sample(t))
    check(lib.bflbm_step(c, 2))

    def geometry():
        g = [ctypes.c_int() for _ in range(4)]
        check(lib.bflbm_shape_geometry(t, *[ctypes.byref(v) for v in g]))
        return [v.value for v in g]

    def read():
        n, b = ctypes.c_longlong(), ctypes.c_int()
        check(lib.bflbm_shape_count(t, ctypes.byref(n), ctypes.byref(b)))
        r = np.empty((n.value, b.value, 3 + len(dirs)))
        steps = np.empty((n.value, b.value), dtype=np.int64)
        check(lib.bflbm_shape_read(t, 0, n.value, r.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.c_void_p)))
        return steps, r

    geo0 = geometry()
    assert geo0[:2] == [len(dirs), 24]
    steps0, r0 = read()
    assert steps0[:, 0].tolist() == [0, 1, 2] and _finite_and_varied(r0[-1, 0, 3:])
    check(lib.bflbm_destroy(c))
    steps1, r1 = read()
    assert np.array_equal(steps0, steps1) and _same(r0, r1) and geometry() == geo0
    assert lib.bflbm_shape_sample(t) != 0
    assert "destroyed" in lib.bflbm_last_error().decode()
    tail = np.empty((1, 1, 3 + len(dirs)))
    check(lib.bflbm_shape_read(t, 2, 1, tail.ctypes.data_as(ctypes.c_void_p), None))      # a window, without labels
    assert _same(tail[0], r0[2])
    assert lib.bflbm_shape_read(t, 2, 2, tail.ctypes.data_as(ctypes.c_void_p), None) != 0
    check(lib.bflbm_shape_destroy(t))
