"""GPU: interface traces (InterfaceTrace, bflbm_iface_*): the rising and falling height of a density contour above every
column of every replica, scanned along z on the device every k steps.

The definition is in include/bflbm.h ("Interface traces"); analysis.interface_heights restates it in numpy.  A sample
must equal that restatement applied to the downloaded density of the same state: the same arithmetic on the same doubles,
so every comparison is exact, with NaNs (columns without a crossing) matched by position.  A trace changes nothing its
owner computes.  The shapes are those of tests/test_gpu_trace.py: a plane smaller than one block, a padded pitch with
several blocks per plane, unequal extents with a ragged last block, nx no multiple of the padding, and a lattice the
hand-over schedule takes."""
import ctypes

import numpy as np
import pytest

from observable_twins import same_doubles as _same

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 8), (24, 24, 24), (20, 28, 24), (72, 12, 10), (64, 8, 16)]
HANDOVER_SHAPE = (64, 8, 16)
# LBM_init_droplet centres the droplet at z = nx / 2 with radius r nx (LBM_binary.H:725): in the two flat boxes radius 0.25
# leaves the droplet outside the lattice, radius 0.4 puts its cap inside.  With these radii the CPU oracle gives, after 2 to
# 5 steps at kBT = 0 and 1e-5, columns with and without a crossing of rho = 0.5 and of phi = 0.5 on every shape (for rho
# 9 of 64, 97 of 576, 69 of 560, 69-138 of 864 and 278-286 of 512 columns cross); each test asserts it on what it compares.
RADIUS = {(8, 8, 8): 0.25, (24, 24, 24): 0.25, (20, 28, 24): 0.25, (72, 12, 10): 0.4, (64, 8, 16): 0.4}
FIELDS = ("rho", "phi")


def _droplet(pkg, n, schedule=None, kBT=0.0, radius=None, steps=2, **params):
    """A droplet as in tests/test_gpu_trace.py (alpha0 = 2.5) after a few steps."""
    p = dict(alpha0=2.5, kBT=kBT)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_droplet(RADIUS[n] if radius is None else radius)
    lbm.LBM_timestep(steps)
    return lbm


def _level(lbm):
    return (lbm.params.rho_hi + lbm.params.rho_lo) / 2


def _densities(lbm):
    """rho, phi [nz, ny, nx] of the resident state: the doubles the kernel forms."""
    return lbm.LBM_hydrovars_density(ncomp=2)


def _both_kinds(h):
    """Columns with and without a crossing, and not one height everywhere."""
    finite = h[~np.isnan(h)]
    return 0 < finite.size < h.size and np.unique(finite).size > 1


# ---- 1. a lone droplet: every sample equals the restatement on a twin without a trace ------------------------------------
CASES = [(n, s, kBT) for n in SHAPES for s in ("two_pass", "fused") for kBT in (0.0, 1e-5)]
CASES += [(HANDOVER_SHAPE, "handover", kBT) for kBT in (0.0, 1e-5)]


@pytest.mark.parametrize("n,schedule,kBT", CASES)
def test_lone_interface_trace_equals_the_restatement(pkg, n, schedule, kBT):
    a = _droplet(pkg, n, schedule, kBT)
    b = _droplet(pkg, n, schedule, kBT)                                  # the twin without a trace
    if schedule == "handover":
        assert a.resolved_schedule() == "handover" and b.resolved_schedule() == "handover"
    level = _level(a)
    moments0 = b.droplet_moments()
    assert np.array_equal(a.droplet_moments(), moments0)
    traces = [a.interface_trace(level, field=f, every=1, capacity=4) for f in FIELDS]    # an owner may carry several
    for tr in traces:
        tr.sample()
    want = [[pkg.analysis.interface_heights(d, level) for d in _densities(b)]]
    for _ in range(3):
        a.LBM_timestep(1)
        b.LBM_timestep(1)
        want.append([pkg.analysis.interface_heights(d, level) for d in _densities(b)])
    for k, tr in enumerate(traces):
        assert tr.count == 4
        assert tr.geometry()[:2] == (n[0], n[1])
        steps, h = tr.read()
        assert steps.shape == (4, 1) and steps.dtype == np.int64 and h.shape == (4, 1, 2, n[1], n[0])
        assert steps[:, 0].tolist() == [2, 3, 4, 5]
        for s in range(4):
            assert _both_kinds(want[s][k]), (FIELDS[k], s)               # the comparison below is about something
            assert _same(h[s, 0], want[s][k]), (FIELDS[k], s)
        assert _same(tr.rising(), h[:, :, 0]) and _same(tr.falling(), h[:, :, 1])
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.droplet_moments(), b.droplet_moments())      # the owner's own reduction is undisturbed
    a.close()
    assert all(tr._h is None for tr in traces)                           # closing the owner closed its dependents
    b.close()


# ---- 2. segments ---------------------------------------------------------------------------------------------------------
def test_segments_change_nothing(pkg):
    """One segment, several segments, a ragged last segment, windows inside the lattice, and a crossing on the first pair
    of a later segment (its lower plane is the last plane of the segment before)."""
    seen = []
    for n, window in [((8, 8, 8), None), ((24, 24, 24), None), ((24, 24, 24), (3, 21)), ((24, 24, 24), (4, 8)),
                      ((72, 12, 10), None), ((20, 28, 24), (2, 23)), ((64, 8, 16), (5, 7))]:
        lbm = _droplet(pkg, n, kBT=1e-5, steps=3)
        level = _level(lbm)
        z_lo, z_hi = (0, n[2]) if window is None else window
        traces = [lbm.interface_trace(level, field=f, window=window, capacity=1) for f in FIELDS]
        nx, ny, nseg, seg_pairs = traces[0].geometry()
        npairs = z_hi - z_lo - 1
        assert (nx, ny) == n[:2] and nseg >= 1 and seg_pairs >= 1
        assert (nseg - 1) * seg_pairs < npairs <= nseg * seg_pairs      # the segments cover the pairs, none is empty
        assert nseg == 1 or seg_pairs >= 4
        if z_hi - z_lo == 4:
            assert nseg == 1                                             # a window of 4 planes: one segment
        seen.append((nseg, npairs % seg_pairs != 0))
        for tr, d in zip(traces, _densities(lbm)):
            tr.sample()
            assert _same(tr.read()[1][0, 0], pkg.analysis.interface_heights(d, level, window)), (n, window)
        lbm.close()
    assert any(s == 1 for s, _ in seen) and any(s > 1 for s, _ in seen) and any(s > 1 and ragged for s, ragged in seen), seen

    # a crossing on the pair that straddles two segments: planes (zs, zs+1) with zs the last plane segment 0 reads
    n = (24, 24, 24)
    lbm = _droplet(pkg, n, steps=3)
    rho = _densities(lbm)[0]
    probe = lbm.interface_trace(_level(lbm), capacity=1)
    _, _, nseg, seg_pairs = probe.geometry()
    probe.close()
    assert nseg > 1
    zs = seg_pairs
    y, x = n[1] // 2, n[0] // 2                                          # the column through the droplet's centre
    assert rho[zs + 1, y, x] != rho[zs, y, x]
    level = float((rho[zs, y, x] + rho[zs + 1, y, x]) / 2)
    tr = lbm.interface_trace(level, capacity=1)
    assert tr.geometry()[2:] == (nseg, seg_pairs)
    tr.sample()
    want = pkg.analysis.interface_heights(rho, level)
    k = 0 if rho[zs + 1, y, x] > rho[zs, y, x] else 1
    assert zs <= want[k, y, x] < zs + 1                                  # the column's first crossing is on that pair
    got = tr.read()[1][0, 0]
    assert got[k, y, x] == want[k, y, x] and _same(got, want)
    lbm.close()


# ---- 3. equality at the level ---------------------------------------------------------------------------------------------
def test_a_density_exactly_at_the_level(pkg):
    """level = the density of one site.  As d(z) it closes a rising pair (h = z exactly); as d(z-1) it opens a falling
    pair (h = z-1 exactly)."""
    n = (24, 24, 24)
    lbm = _droplet(pkg, n, steps=3)
    rho = _densities(lbm)[0]
    y, x = n[1] // 2, n[0] // 2
    col = rho[:, y, x]
    z_up = int(np.argmax(col > 0.5))                                     # the first plane above 0.5: on the rising flank
    z_dn = int(len(col) - 1 - np.argmax(col[::-1] > 0.5))                # the last plane above 0.5: on the falling flank
    assert 0 < z_up < z_dn < n[2] - 1 and col[z_up - 1] < col[z_up] and col[z_dn] > col[z_dn + 1]
    for z0, k in ((z_up, 0), (z_dn, 1)):
        level = float(col[z0])
        tr = lbm.interface_trace(level, capacity=1)
        tr.sample()
        want = pkg.analysis.interface_heights(rho, level)
        assert want[k, y, x] == float(z0)                                # the equality case is in play
        got = tr.read()[1][0, 0]
        assert got[k, y, x] == float(z0) and _same(got, want)
        tr.close()
    lbm.close()


# ---- 4. no crossing at all ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(8, 8, 8), (72, 12, 10)])
def test_a_level_above_the_field_gives_nan_everywhere(pkg, n):
    lbm = _droplet(pkg, n, kBT=1e-5)
    d = _densities(lbm)
    level = float(max(d[0].max(), d[1].max())) + 1.0
    for f in FIELDS:
        tr = lbm.interface_trace(level, field=f, capacity=1)
        tr.sample()
        h = tr.read()[1]
        assert h.shape == (1, 1, 2, n[1], n[0]) and np.isnan(h).all()
    lbm.close()


# ---- 5. a batch records what lone lattices give ---------------------------------------------------------------------------
REPLICAS = [dict(alpha0=2.5, kappa=4.0, seed=11), dict(alpha0=2.0, kappa=2.0, seed=12), dict(alpha0=1.5, kappa=1.0, seed=13),
            dict(alpha0=2.2, kappa=3.0, seed=14), dict(alpha0=1.0, kappa=0.5, seed=15)]
RADII = [0.25, 0.2, 0.3, 0.15, 0.35]


def _batch(pkg, n, nrep, schedule, kBT=1e-5):
    params = [dict(p, kBT=kBT) for p in REPLICAS[:nrep]]
    batch = pkg.BatchLBM(n, params=params, schedule=schedule)
    for lat, r in zip(batch.replicas, RADII):
        lat.LBM_init_droplet(r)
    return batch


def _lones(pkg, n, nrep, schedule, kBT=1e-5):
    lones = [pkg.BinaryLBM(*n, params=pkg.default_params(**dict(p, kBT=kBT)), schedule=schedule) for p in REPLICAS[:nrep]]
    for lat, r in zip(lones, RADII):
        lat.LBM_init_droplet(r)
    return lones


@pytest.mark.parametrize("n,nrep,schedule", [((24, 24, 24), 5, "two_pass"), ((24, 24, 24), 5, "fused"),
                                             ((20, 28, 24), 1, "two_pass"), ((20, 28, 24), 1, "fused"),
                                             ((20, 28, 24), 3, "two_pass"), ((20, 28, 24), 3, "fused")])
def test_batch_interface_trace_equals_lone_lattices(pkg, n, nrep, schedule):
    batch, twin, lones = _batch(pkg, n, nrep, schedule), _batch(pkg, n, nrep, schedule), _lones(pkg, n, nrep, schedule)
    assert batch.resolved_schedule() == schedule
    level = 0.5
    t1 = batch.interface_trace(level, field="rho", every=1, capacity=8)
    t3 = batch.interface_trace(level, field="phi", every=3, capacity=2)
    t1.sample()

    def observe():
        d = [_densities(lone) for lone in lones]
        return ([lone.steps_done for lone in lones],
                np.array([pkg.analysis.interface_heights(x[0], level) for x in d]),
                np.array([pkg.analysis.interface_heights(x[1], level) for x in d]))

    want = {0: observe()}
    again = nrep - 1                                                     # re-initialised after one step: its resident state
    for s in range(1, 8):                                                # then sits in the other buffer than its neighbours'
        batch.LBM_timestep(1)
        twin.LBM_timestep(1)
        for lone in lones:
            lone.LBM_timestep(1)
        want[s] = observe()
        if s == 1:
            for owner in (batch.replicas, twin.replicas, lones):
                owner[again].LBM_init_droplet(RADII[again])
    assert t1.count == 8 and t3.count == 2
    steps, h = t1.read()
    assert h.shape == (8, nrep, 2, n[1], n[0])
    for s in range(8):
        assert steps[s].tolist() == want[s][0], s
        assert _both_kinds(want[s][1]) and _same(h[s], want[s][1]), s
    assert steps[-1].tolist() == [7] * (nrep - 1) + [6]                  # the re-initialised replica counts from its init
    steps, h = t3.read()
    for k, s in enumerate((3, 6)):
        assert steps[k].tolist() == want[s][0]
        assert _both_kinds(want[s][2]) and _same(h[k], want[s][2]), s
    for u, v in zip(batch.populations(), twin.populations()):
        assert np.array_equal(u, v)
    for lat in [batch, twin] + lones:
        lat.close()


# ---- 6. several observers on one batch -------------------------------------------------------------------------------------
def test_two_interface_traces_and_a_moments_trace_on_one_batch(pkg):
    n, nrep, level = (24, 24, 24), 3, 0.5
    makers = [lambda b: b.interface_trace(level, field="rho", every=1, capacity=5),
              lambda b: b.interface_trace(level, field="phi", every=2, capacity=5),
              lambda b: b.trace(every=1, capacity=5, threshold=0.06)]
    together = _batch(pkg, n, nrep, None)
    observers = [make(together) for make in makers]
    for ob in observers:
        ob.sample()
    together.LBM_timestep(4)
    got = [ob.read() for ob in observers]
    assert [len(g[0]) for g in got] == [5, 3, 5]
    for make, g in zip(makers, got):
        alone = _batch(pkg, n, nrep, None)
        ob = make(alone)
        ob.sample()
        alone.LBM_timestep(4)
        steps, rec = ob.read()
        assert np.array_equal(steps, g[0]) and _same(rec, g[1])
        alone.close()
    together.close()


# ---- 7. the notebook's geometry, small -------------------------------------------------------------------------------------
def test_flat_interface_stripes(pkg):
    """4 x (8, 64, 32) stripes with the parameters of Flat_Interface.ipynb at kBT = 1e-5, 200 steps sampled every 20.  The
    stripe fills every column: the CPU oracle, run with these parameters and the four seeds for 200 steps, finds a falling
    crossing of rho = 1.55 in every column of every sample (heights 23.57 ... 24.0), so no NaN is allowed here.  No physics
    band is asserted; the long statistical run is tests/test_gpu_notebook_noise.py."""
    n, nrep, level = (8, 64, 32), 4, 1.55
    batch = pkg.BatchLBM(n, params=dict(alpha0=1.5, rho_lo=0.1, rho_hi=3.0, kappa=0.1, kBT=1e-5), replicas=nrep)
    for rep in batch.replicas:
        rep.LBM_init_stripe(0.5)
    tr = batch.interface_trace(level, every=20, capacity=10)
    want = []
    for _ in range(10):
        batch.LBM_timestep(20)
        rho = batch.LBM_hydrovars_density(ncomp=1)[:, 0]
        want.append([pkg.analysis.interface_heights(rho[r], level)[1] for r in range(nrep)])
    steps, h = tr.read()
    assert steps.tolist() == [[20 * (k + 1)] * nrep for k in range(10)]
    falling = tr.falling()
    assert falling.shape == (10, nrep, n[1], n[0]) and _same(falling, h[:, :, 1])
    assert not np.isnan(falling).any()
    assert np.array_equal(falling, np.array(want))
    assert np.unique(falling).size > 1000                                # a fluctuating interface, not one number
    spectrum, (qy, qx) = pkg.analysis.capillary_spectrum(falling, axes=(-2, -1))     # time first: all replicas at once
    assert spectrum.shape == (nrep, n[1], n[0]) and np.isfinite(spectrum).all() and (spectrum >= 0).all()
    assert qy.shape == (n[1],) and qx.shape == (n[0],)
    line, (q,) = pkg.analysis.capillary_spectrum(falling[:, 0, :, 4], axes=(-1,))    # the notebook's one x-line
    assert line.shape == (n[1],) and np.array_equal(q, qy)
    batch.close()


# ---- 8. rules ---------------------------------------------------------------------------------------------------------------
# every = 2, capacity = 3 (the protocol of tests/test_gpu_trace.py): 7 steps from a fresh trace add the samples of steps 2, 4
# and 6, which fit; 8 steps do not.
def _overflow_protocol(pkg, owner, steps_done):
    first = owner.interface_trace(0.5, every=1, capacity=64)             # served first; must not be touched by a refusal
    tr = owner.interface_trace(0.5, field="phi", every=2, capacity=3)
    state = owner.populations()
    with pytest.raises(pkg.BflbmError, match="interface trace full"):
        owner.LBM_timestep(8)                                            # samples at 2, 4, 6, 8
    assert steps_done() == 0 and tr.count == 0 and first.count == 0
    assert all(np.array_equal(u, v) for u, v in zip(state, owner.populations()))
    owner.LBM_timestep(6)
    assert tr.count == 3 and first.count == 6
    with pytest.raises(pkg.BflbmError, match="interface trace full"):
        tr.sample()
    assert tr.count == 3
    tr.reset()                                                           # reset restarts the count of steps as well
    assert tr.count == 0 and first.count == 6
    owner.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="interface trace full"):
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
    with pytest.raises(pkg.BflbmError, match="interface trace full"):
        lbm.step_boundary()                                              # the eighth step would sample
    with pytest.raises(pkg.BflbmError, match="bflbm_step_boundary first"):
        lbm.step_interior()                                              # the refused step is not open
    assert lbm.steps_done == 13 and tr.count == 3
    assert all(np.array_equal(u, v) for u, v in zip(state, lbm.populations()))
    lbm.close()


def test_overflow_is_refused_before_any_launch_batch(pkg):
    batch = _batch(pkg, (24, 24, 24), 3, None, kBT=0.0)
    _overflow_protocol(pkg, batch, lambda: max(r.steps_done for r in batch.replicas))
    assert [r.steps_done for r in batch.replicas] == [13, 13, 13]
    batch.close()


def test_creation_refusals(pkg):
    lib = pkg._lib.load()

    def refused(create, handle, pattern, field=0, level=0.5, z_lo=0, z_hi=8, every=1, capacity=4):
        h = ctypes.c_void_p()
        rc = getattr(lib, create)(handle, field, level, z_lo, z_hi, every, capacity, ctypes.byref(h))
        msg = lib.bflbm_last_error().decode()
        assert rc != 0 and not h.value, (create, pattern)
        assert pattern in msg and create in msg, msg

    lbm = _droplet(pkg, (8, 8, 8), steps=0)
    batch = _batch(pkg, (8, 8, 8), 2, None)
    for create, owner in (("bflbm_iface_create", lbm), ("bflbm_batch_iface_create", batch)):
        assert getattr(lib, create)(owner._h, 0, 0.5, 0, 8, 1, 4, None) != 0             # a valid owner, no place for the handle
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and create in msg, msg
        refused(create, owner._h, "field", field=2)
        refused(create, owner._h, "field", field=-1)
        refused(create, owner._h, "NaN", level=float("nan"))
        refused(create, owner._h, "window", z_lo=-1)
        refused(create, owner._h, "window", z_hi=9)
        refused(create, owner._h, "window", z_lo=4, z_hi=5)
        refused(create, owner._h, "every", every=0)
        refused(create, owner._h, "capacity", capacity=0)
        refused(create, owner._h, "1 TB", capacity=1 << 40)
    refused("bflbm_iface_create", batch.replicas[0]._h, "bflbm_batch_iface_create")
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_iface_create"):
        batch.replicas[0].interface_trace(0.5)
    with pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2) as slab:
        refused("bflbm_iface_create", slab._h, "nranks > 1")
    with pytest.raises(ValueError):
        lbm.interface_trace(0.5, field="density")
    # an open step refuses creation, and sample / reset / read of an existing trace
    tr = lbm.interface_trace(0.5, window=(2, 6), capacity=4)
    tr.sample()
    lbm.step_boundary()
    refused("bflbm_iface_create", lbm._h, "open step")
    for call in (tr.sample, tr.reset, tr.read):
        with pytest.raises(pkg.BflbmError, match="open step"):
            call()
    assert tr.count == 1
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2                                                 # the split step samples in its finish
    assert tr.read()[0][:, 0].tolist() == [0, 1]
    for lat in (lbm, batch):
        lat.close()


def test_interface_trace_outlives_its_owner(pkg):
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
    check(lib.bflbm_iface_create(c, 0, 0.5, 0, 24, 1, 8, ctypes.byref(t)))
    check(lib.bflbm_iface_sample(t))
    check(lib.bflbm_step(c, 2))

    def geometry():
        g = [ctypes.c_int() for _ in range(4)]
        check(lib.bflbm_iface_geometry(t, *[ctypes.byref(v) for v in g]))
        return [v.value for v in g]

    def read():
        n, b = ctypes.c_longlong(), ctypes.c_int()
        check(lib.bflbm_iface_count(t, ctypes.byref(n), ctypes.byref(b)))
        h = np.empty((n.value, b.value, 2, 24, 24))
        steps = np.empty((n.value, b.value), dtype=np.int64)
        check(lib.bflbm_iface_read(t, 0, n.value, h.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.c_void_p)))
        return steps, h

    geo0 = geometry()
    steps0, h0 = read()
    assert steps0[:, 0].tolist() == [0, 1, 2] and _both_kinds(h0[-1, 0])
    check(lib.bflbm_destroy(c))
    steps1, h1 = read()
    assert np.array_equal(steps0, steps1) and _same(h0, h1) and geometry() == geo0
    assert lib.bflbm_iface_sample(t) != 0
    assert "destroyed" in lib.bflbm_last_error().decode()
    tail = np.empty((1, 1, 2, 24, 24))
    check(lib.bflbm_iface_read(t, 2, 1, tail.ctypes.data_as(ctypes.c_void_p), None))     # a window, without labels
    assert _same(tail[0], h0[2])
    assert lib.bflbm_iface_read(t, 2, 2, tail.ctypes.data_as(ctypes.c_void_p), None) != 0
    check(lib.bflbm_iface_destroy(t))


def test_closing_a_batch_closes_its_interface_traces(pkg):
    batch = _batch(pkg, (8, 8, 8), 2, None)
    tr = batch.interface_trace(0.5, capacity=2)
    tr.sample()
    assert tr.count == 1
    batch.close()
    assert tr._h is None
