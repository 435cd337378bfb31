"""GPU: radial traces (RadialTrace, bflbm_radial_*): the sums of chosen hydrodynamic variables, of products of them and of
projections onto the radial unit vector over the shells about a droplet's centre, recorded on the device.

The definition and the order of the sums are in include/bflbm.h ("Radial traces"); tests/radial_sums.py writes that
order out site by site (emulate), and tests/test_radial_abi.py holds the numpy twin to it and to the exact sums.  Here
the device record is compared with the emulation of the downloaded fields bit for bit: lone lattices and replicas of a
batch, fixed centres and the centre of mass.  The golden droplets carry the oracle's figures (make_golden_radial.py)."""
import ctypes
import os

import numpy as np
import pytest

import radial_sums as rs

pytestmark = pytest.mark.gpu

HYD = ["rho", "afx", "afy", "afz", "phi"]                  # of hydrovs; NV = 5
HYD_PAIRS = [("rho", "phi"), ("afz", "afz")]
HYD_RADIALS = [(None, ("afx", "afy", "afz")), ("rho", ("afx", "afy", "afz"))]
BAR = ["phi", "rho", "ufx"]                                # of hydrovsbar, not in ascending order; NV = 3
BAR_PAIRS = [("phi", "rho")]
BAR_RADIALS = [("phi", ("ufx", "rho", "phi"))]
DELTA = 0.75
THRESHOLD = 0.06
BOXES = rs.BOXES + [(16, 16, 16)]


def _start(o, n):
    """A droplet where the box holds one, a stripe in the thin boxes; kBT = 1e-5 leaves no shell uniform."""
    if min(n) >= 5:
        o.LBM_init_droplet(0.3)
    else:
        o.LBM_init_stripe(0.5)


def _lone(pkg, n, schedule=None, **params):
    p = dict(kBT=1e-5, alpha0=2.5, seed=7)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    _start(lbm, n)
    return lbm


def _params():
    return [dict(alpha0=a, kappa=k, tau_f=t, tau_g=t, kBT=kbt, seed=s)
            for a, k, t, kbt, s in zip((2.5, 1.5, 2.0), (4.0, 0.1, 2.0), (0.5, 0.8, 1.0), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


def _batch(pkg, n, schedule=None):
    """Three replicas that differ in parameters, seed and step counter."""
    batch = pkg.BatchLBM(n, params=_params(), schedule=schedule)
    for v in batch.replicas:
        _start(v, n)
    batch.replicas[1].set_steps_done(1000)
    return batch


def _slots(names, pairs, radials):
    return ([(names.index(a), names.index(b)) for a, b in pairs],
            [(None if w is None else names.index(w), tuple(names.index(c) for c in v)) for w, v in radials])


def _index(pkg, names, bar):
    all_names = pkg.plotfile.variable_names(9 if bar else 22)
    return [all_names.index(v) for v in names]


def _traces(o, n, centres, **kw):
    """{(source, centre name): trace}: hydrovs about every fixed centre and about the centre of mass, hydrovsbar about
    the first fixed centre and about the centre of mass."""
    out = {}
    for name, c in centres.items():
        out[("hydrovs", name)] = o.radial_trace(HYD, HYD_PAIRS, HYD_RADIALS, centre=c, delta=DELTA, **kw)
    first = next(iter(centres))
    out[("hydrovsbar", first)] = o.radial_trace(BAR, BAR_PAIRS, BAR_RADIALS, centre=centres[first], delta=DELTA, source="hydrovsbar", **kw)
    out[("hydrovs", "com")] = o.radial_trace(HYD, HYD_PAIRS, HYD_RADIALS, threshold=THRESHOLD, delta=DELTA, **kw)
    out[("hydrovsbar", "com")] = o.radial_trace(BAR, BAR_PAIRS, BAR_RADIALS, threshold=THRESHOLD, delta=DELTA, source="hydrovsbar", nbins=5, **kw)
    return out


def _want(pkg, lattice, n, key, centre, nbins):
    """emulate of the lattice's downloaded fields about `centre`: (counts, sums)."""
    if key[0] == "hydrovs":
        fields = lattice.LBM_hydrovars()[_index(pkg, HYD, False)]
        ps, rd = _slots(HYD, HYD_PAIRS, HYD_RADIALS)
    else:
        fields = lattice.LBM_hydrovars_density()[_index(pkg, BAR, True)]
        ps, rd = _slots(BAR, BAR_PAIRS, BAR_RADIALS)
    return fields, ps, rd, rs.emulate(fields, centre, DELTA, nbins, ps, rd)


def _fixed(n):
    return {k: v for k, v in rs.centres(n).items() if k != "nan"}          # a NaN fixed centre is refused; see the threshold test


# ---- 1. against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES)
def test_lone_record_equals_the_emulation(pkg, n):
    lbm = _lone(pkg, n)
    lbm.LBM_timestep(3)
    moments = lbm.trace(every=1, capacity=1, threshold=THRESHOLD)
    shape = lbm.shape_trace(0.5, pkg.analysis.ray_nodes(2, 4), threshold=THRESHOLD, capacity=1)
    traces = _traces(lbm, n, _fixed(n), capacity=1)
    moments.sample(); shape.sample()
    for tr in traces.values():
        tr.sample()
    com = moments.com()[0, 0]
    assert np.isfinite(com).all() and np.array_equal(shape.read()[1][0, 0], com)
    for key, tr in traces.items():
        nq = 9 if key[0] == "hydrovs" else 5
        nbins = 5 if key == ("hydrovsbar", "com") else rs.default_bins(n, DELTA)
        assert tr.geometry() == rs.geometry(n, nq, nbins), key
        centres, counts, sums, steps = tr.read()
        assert centres.shape == (1, 1, 3) and counts.shape == (1, 1, nbins) and sums.shape == (1, 1, nq, nbins)
        assert steps.tolist() == [[3]] and steps.dtype == np.int64
        want_centre = com if key[1] == "com" else np.array(rs.centres(n)[key[1]])
        assert np.array_equal(centres[0, 0], want_centre), (n, key)          # Trace.com() and the shape trace's, bit for bit
        fields, ps, rd, (w_counts, w_sums) = _want(pkg, lbm, n, key, centres[0, 0], nbins)
        assert np.array_equal(counts[0, 0], w_counts), (n, key)
        assert np.array_equal(sums[0, 0], w_sums), (n, key, np.abs(sums[0, 0] - w_sums).max())
        twin = pkg.analysis.radial_shells(fields, centres[0, 0], DELTA, nbins, ps, rd)
        assert np.array_equal(counts[0, 0], twin[0]) and np.array_equal(sums[0, 0], twin[1]), (n, key)
        assert counts.sum() == n[0] * n[1] * n[2] if nbins != 5 else 0 < counts.sum() < n[0] * n[1] * n[2]
        assert np.count_nonzero(sums[0, 0, 0]) > 1 and np.count_nonzero(sums[0, 0, -1]) > 1     # no empty record
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.array_equal(tr.means()[0, 0], np.where(counts[0, 0] > 0, sums[0, 0] / counts[0, 0], np.nan), equal_nan=True)
        assert np.array_equal(tr.r, (np.arange(nbins) + 0.5) * DELTA)
    assert traces[("hydrovs", "com")].names == HYD and traces[("hydrovsbar", "com")].names == BAR
    lbm.close()


def test_a_threshold_above_every_density_gives_an_empty_record(pkg):
    n = (16, 16, 16)
    for owner in (_lone(pkg, n), _batch(pkg, n)):
        owner.LBM_timestep(1)
        tr = owner.radial_trace(HYD, HYD_PAIRS, HYD_RADIALS, threshold=1e3, capacity=1)
        tr.sample()
        centres, counts, sums, _ = tr.read()
        assert np.isnan(centres).all() and not counts.any() and not sums.any() and not np.signbit(sums).any()
        assert np.isnan(tr.means()).all()
        owner.close()


@pytest.mark.parametrize("n", BOXES)
def test_batch_record_equals_the_emulation_and_the_lattice_run_alone(pkg, n):
    centres = {"corner": rs.centres(n)["corner"]}
    batch = _batch(pkg, n)
    batch.LBM_timestep(3)
    traces = _traces(batch, n, centres, capacity=1)
    for tr in traces.values():
        tr.sample()
    got = {key: tr.read() for key, tr in traces.items()}
    for r, v in enumerate(batch.replicas):
        for key, (c, counts, sums, steps) in got.items():
            assert steps.tolist() == [[3, 1003, 3]] and sums.shape[:2] == (1, 3)
            _, _, _, (w_counts, w_sums) = _want(pkg, v, n, key, c[0, r], counts.shape[-1])
            assert np.array_equal(counts[0, r], w_counts) and np.array_equal(sums[0, r], w_sums), (n, key, r)
    assert not np.array_equal(got[("hydrovs", "com")][0][0, 0], got[("hydrovs", "com")][0][0, 1])      # every replica its own centre
    batch.close()
    for r, p in enumerate(_params()):
        lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p))
        _start(lbm, n)
        if r == 1:
            lbm.set_steps_done(1000)
        lbm.LBM_timestep(3)
        alone = _traces(lbm, n, centres, capacity=1)
        for key, tr in alone.items():
            tr.sample()
            for a, b in zip(tr.read(), got[key]):
                assert np.array_equal(a[0, 0], b[0, r]), (n, key, r)
        lbm.close()


def test_batch_centre_at_frame_zero_equals_the_trace(pkg):
    """Frame 0, before any step, is when the batch's record table is stale: the radial trace's centre-of-mass launch must
    bring the table up to date itself, whatever was sampled before it.  The box: the smallest of radial_sums.BOXES whose
    plane is no multiple of 256 sites."""
    n = min((b for b in rs.BOXES if (b[0] * b[1]) % 256), key=lambda b: b[0] * b[1] * b[2])
    batch = pkg.BatchLBM(n, params=_params()[:2])
    for v in batch.replicas:
        _start(v, n)
    radial = batch.radial_trace(["rho"], threshold=THRESHOLD, capacity=1)
    moments = batch.trace(every=1, capacity=1, threshold=THRESHOLD)
    radial.sample(); moments.sample()
    centres, _, _, steps = radial.read()
    com = moments.com()
    assert steps.tolist() == [[0, 0]] and centres.shape == com.shape == (1, 2, 3)
    assert np.isfinite(com).all() and centres.tobytes() == com.tobytes()
    batch.close()


# ---- 2. automatic sampling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n = (9, 7, 5)
    o = _lone(pkg, n) if owner == "lone" else _batch(pkg, n)
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: max(v.steps_done for v in o.replicas) - 1000)
    other = o.trace(every=1, capacity=16)
    tr = o.radial_trace(["rho", "phi"], [("rho", "phi")], threshold=THRESHOLD, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="radial trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    assert tr.count == 1 and tr.read()[3][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    rec = tr.read()
    steps = rec[3]
    with pytest.raises(pkg.BflbmError, match="radial trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="radial trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    assert all(np.array_equal(a, b) for a, b in zip(rec, tr.read()))
    assert (steps[:, 0] - steps[0, 0]).tolist() == [0, 1, 2] and steps[0, 0] == 2
    assert not np.array_equal(rec[2][0], rec[2][1]) and not np.array_equal(rec[2][1], rec[2][2])
    assert all(np.array_equal(a, b[1:]) for a, b in zip(tr.read(first=1, count=2), rec))      # a window of the record
    tr.reset()
    assert tr.count == 0 and tr.read()[2].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[3][0, 0] == 7
    # the owner goes first: the trace stays readable with the same bits, refuses a sample, closes twice
    rec = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    assert all(np.array_equal(a, b) for a, b in zip(rec, tr.read())) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_radial_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lone(pkg, (9, 7, 5))
    t = ctypes.c_void_p()
    va, pa, pb = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    rw, rv = (ctypes.c_int * 1)(-1), (ctypes.c_int * 3)(0, 1, 0)
    c = (ctypes.c_double * 3)(4.25, 3.5, 2.0)
    check(lib.bflbm_radial_create(lbm._h, 1, 2, va, 1, pa, pb, 1, rw, rv, c, 0.0, 1.5, 4, 1, 4, ctypes.byref(t)))
    lbm.LBM_timestep(3)
    per = 3 + 5 * 4

    def read(first, count):
        rec, steps = np.empty((count, 1, per)), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_radial_read(t, first, count, rec.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return rec, steps
    rec0, steps0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3] and np.array_equal(rec0[:, 0, :3], np.tile([4.25, 3.5, 2.0], (3, 1)))
    fields = lbm.LBM_hydrovars_density()[:2]
    counts, sums = rs.emulate(fields, (4.25, 3.5, 2.0), 1.5, 4, [(0, 1)], [(None, (0, 1, 0))])
    assert np.array_equal(rec0[2, 0], rs.record((4.25, 3.5, 2.0), counts, sums))
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    rec1, steps1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(rec0, rec1)
    assert np.array_equal(read(2, 1)[0][0], rec0[2])       # a window
    assert lib.bflbm_radial_read(t, 2, 2, rec0.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.bflbm_radial_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_radial_destroy(t))


# ---- 3. independence of what else is attached ------------------------------------------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders(pkg):
    n = (13, 10, 6)
    modes = np.array([(1, 0, 0), (0, 1, 1)])
    records = []
    for order in ("alone", "first", "last"):
        lbm = _lone(pkg, n, schedule="fused")
        mt = fs = None
        if order == "last":
            fs = lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1)
            mt = lbm.mode_trace(["rho", "ubx"], modes, every=1, capacity=8)
        tr = lbm.radial_trace(HYD, HYD_PAIRS, HYD_RADIALS, threshold=THRESHOLD, every=2, capacity=3)
        if order == "first":
            mt = lbm.mode_trace(["rho", "ubx"], modes, every=1, capacity=8)
            fs = lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1)
        lbm.LBM_timestep(6)
        assert order == "alone" or (mt.count == 6 and fs.count == 6)
        records.append(tr.read() + ((mt.read()[1], fs.cov(0)) if mt else ()))
        lbm.close()
    first = records[0]
    assert first[3][:, 0].tolist() == [2, 4, 6] and not np.array_equal(first[2][0], first[2][2])
    for rec in records[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(rec[:4], first))
    # nor do the others' records depend on where the radial trace stands
    assert np.array_equal(records[1][4], records[2][4]) and np.array_equal(records[1][5], records[2][5])


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm, batch = _lone(pkg, n), _batch(pkg, n)
    nan, inf = float("nan"), float("inf")
    with pytest.raises(pkg.BflbmError, match=r"bflbm_radial_create.*replica of a batch.*use bflbm_batch_radial_create"):
        batch.replicas[0].radial_trace(["rho"])
    lib = pkg._lib.load()

    def raw(owner, call, source=0, nvars=1, variables=(0,), pairs=(), radials=(), centre=None, threshold=0.06, delta=1.0, nbins=4,
            every=1, capacity=4):
        """Past the wrapper's own checks: through the ABI."""
        h = ctypes.c_void_p()
        va = (ctypes.c_int * max(len(variables), 1))(*variables)
        pa = (ctypes.c_int * max(len(pairs), 1))(*[p[0] for p in pairs])
        pb = (ctypes.c_int * max(len(pairs), 1))(*[p[1] for p in pairs])
        rw = (ctypes.c_int * max(len(radials), 1))(*[w for w, _ in radials])
        rv = (ctypes.c_int * max(3 * len(radials), 1))(*[c for _, v in radials for c in v])
        c = None if centre is None else (ctypes.c_double * 3)(*centre)
        pkg._lib.check(getattr(lib, call)(owner._h, source, nvars, va, len(pairs), pa, pb, len(radials), rw, rv, c, threshold, delta, nbins,
                                          every, capacity, ctypes.byref(h)))
        return h

    for owner, call in ((lbm, "bflbm_radial_create"), (batch, "bflbm_batch_radial_create")):
        nrep = 3 if owner is batch else 1
        for pattern, kw in (("variable index 22 outside hydrovs", dict(nvars=2, variables=(0, 22))),
                            ("variable index -1 outside hydrovs", dict(variables=(-1,))),
                            ("variable index 9 outside hydrovsbar", dict(variables=(9,), source=1)),
                            ("variable index 3 given twice", dict(nvars=3, variables=(3, 1, 3))),
                            ("1..8 variables", dict(nvars=9, variables=tuple(range(9)))),
                            ("1..8 variables", dict(nvars=0)),
                            ("0..16 pairs", dict(pairs=[(0, 0)] * 17)),
                            ("0..4 radial terms", dict(radials=[(-1, (0, 0, 0))] * 5)),
                            ("pair 1: slot 2 outside the 2 variables", dict(nvars=2, variables=(0, 1), pairs=[(0, 1), (2, 0)])),
                            ("pair 0: slot -1 outside the 1 variables", dict(pairs=[(0, -1)])),
                            ("radial term 0: weight slot -2 outside", dict(radials=[(-2, (0, 0, 0))])),
                            ("radial term 0: weight slot 1 outside", dict(radials=[(1, (0, 0, 0))])),
                            ("radial term 1: slot 1 outside the 1 variables", dict(radials=[(-1, (0, 0, 0)), (0, (0, 1, 0))])),
                            ("radial term 0: slot -1 outside", dict(radials=[(0, (-1, 0, 0))])),
                            ("source must be 0", dict(source=2)),
                            ("fixed centre is not finite", dict(centre=(1.0, nan, 1.0))),
                            ("fixed centre is not finite", dict(centre=(inf, 1.0, 1.0))),
                            ("threshold is NaN", dict(threshold=nan)),
                            ("delta must be finite and > 0", dict(delta=0.0)),
                            ("delta must be finite and > 0", dict(delta=-1.0)),
                            ("delta must be finite and > 0", dict(delta=inf)),
                            ("delta must be finite and > 0", dict(delta=nan)),
                            ("1..128 shells", dict(nbins=0)),
                            ("1..128 shells", dict(nbins=129)),
                            ("every must be >= 1", dict(every=0)),
                            ("capacity must be >= 1", dict(capacity=0)),
                            ("exceeds 1 TB", dict(capacity=(1 << 37) // ((3 + 2 * 4) * nrep) + 1))):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                raw(owner, call, **kw)
            assert call in str(e.value), (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        with pytest.raises(pkg.BflbmError, match="every must be >= 1") as e:                   # the wrapper reaches the same call
            owner.radial_trace(["rho"], every=0)
        assert call in str(e.value)
        # what is accepted at the edges: a NaN threshold beside a fixed centre, w = -1, and the limits themselves
        edge = raw(owner, call, centre=(1.0, 2.0, 3.0), threshold=nan, radials=[(-1, (0, 0, 0))])
        pkg._lib.check(lib.bflbm_radial_destroy(edge))
        full = owner.radial_trace(list(range(8)), [(k % 8, (3 * k) % 8) for k in range(16)],
                                  [(None, (0, 1, 2)), (3, (4, 5, 6)), (7, (7, 7, 7)), (0, (2, 1, 0))], threshold=THRESHOLD, delta=0.05, nbins=128, capacity=1)
        full.sample()
        centres, counts, sums, _ = full.read()
        assert full.geometry() == (28, 128, 256, 1) and np.isfinite(sums).all() and np.isfinite(centres).all() and counts.sum() > 0
        if owner is lbm:                                   # the limits against the definition too
            x = lbm.LBM_hydrovars()[:8]
            w = rs.emulate(x, centres[0, 0], 0.05, 128, [(k % 8, (3 * k) % 8) for k in range(16)],
                           [(None, (0, 1, 2)), (3, (4, 5, 6)), (7, (7, 7, 7)), (0, (2, 1, 0))])
            assert np.array_equal(counts[0, 0], w[0]) and np.array_equal(sums[0, 0], w[1])
        full.close()
    for bad in (lambda: lbm.radial_trace(["no_such_variable"]), lambda: lbm.radial_trace(["rho"], [("phi", "rho")]),
                lambda: lbm.radial_trace(["rho"], radials=[("rho", ("rho", "rho"))]), lambda: lbm.radial_trace(["rho"], source="noise"),
                lambda: lbm.radial_trace(["rho"], delta=0.0)):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_radial_create inside an open step"):
        lbm.radial_trace(["rho"])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.radial_trace(["rho"], capacity=2)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[3][:, 0].tolist() == [1, 2]       # the split step samples in its finish
    lbm.close(); batch.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_radial_create.*nranks > 1"):
        slab.radial_trace(["rho"])
    slab.close()


# ---- 5. the four golden droplets as one batch ---------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_droplets.npz")
CASES = [("a15_k01_r20", 1.5, 0.1, 0.20), ("a15_k01_r30", 1.5, 0.1, 0.30), ("a17_k10_r20", 1.7, 1.0, 0.20), ("a17_k10_r28", 1.7, 1.0, 0.28)]


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_golden_droplets_as_one_batch(pkg, schedule):
    """Four of Surface_Tension.ipynb's 32^3 droplets (rho_hi = 3, tau = 1/2, kBT = 0) as ONE batch with per-replica
    parameters, 20000 steps: one sample of the Laplace inputs about the centre of mass of the cells above 0.06 equals the
    CPU oracle's record (tests/golden/radial_droplets.npz, make_golden_radial.py) bit for bit, and with it Delta p, the
    force integral and the two-point Laplace slope / 2; the radius of the iterative fit to 1e-9.  The oracle gives
        a15_k01_r20  Delta p 0.127976456626  R 0.176078638      a15_k01_r30  Delta p 0.0812020565863  R 0.283804828
        a17_k10_r20  Delta p 0.144761874881  R 0.193161409      a17_k10_r28  Delta p 0.104630934218   R 0.270776076
        slope / 2:   a15_k01 0.0108488417953 (notebook 0.0107839), a17_k10 0.0135218527274 (notebook 0.0134573)
    tests/test_radial_abi.py holds these against the notebook's numbers."""
    golden = {k.replace("__", "/"): v for k, v in np.load(GOLDEN).items()}
    n = tuple(int(v) for v in golden["shape"])
    nbins = int(golden["nbins"])
    an = pkg.analysis
    names, pairs, radials = an.laplace_inputs()
    params = [dict(rho_hi=3.0, rho_lo=0.0, tau_f=0.5, tau_g=0.5, kBT=0.0, alpha0=a, kappa=k) for _, a, k, _ in CASES]
    batch = pkg.BatchLBM(n, params=params, schedule=schedule)
    for v, (_, _, _, r) in zip(batch.replicas, CASES):
        v.LBM_init_droplet(r)
    batch.LBM_timestep(int(golden["steps"]))
    tr = batch.radial_trace(names, pairs, radials, threshold=0.06, delta=1.0, capacity=1)
    tr.sample()
    centres, counts, sums, steps = tr.read()
    assert steps.tolist() == [[int(golden["steps"])] * 4] and tr.names == names and tr.geometry() == rs.geometry(n, 11, nbins)
    means = tr.means()[0]
    found = {}
    for k, (case, alpha0, _, _) in enumerate(CASES):
        rec = rs.record(centres[0, k], counts[0, k], sums[0, k])
        dp = float(an.pressure_jump(an.radial_pressure(means[k], names, alpha0, 1.0 / 3.0), counts[0, k], tr.r, 3.0, 16.0))
        force = float(an.radial_force_integral(means[k], names, 1.0, n[0]))
        R = an.fit_radial_profile(tr.r, means[k, 0], counts[0, k])[2] / n[0]
        print("%s %s: centre %s, Delta p %.12g (oracle %.12g), force integral %.12g (oracle %.12g), R %.9f (oracle %.9f)"
              % (case, schedule, centres[0, k], dp, float(golden["dp/" + case]), force, float(golden["force/" + case]), R, float(golden["R/" + case])))
        assert np.array_equal(rec[:3], golden["centre/" + case]), case
        assert np.array_equal(rec, golden["rec/" + case]), (case, np.abs(rec - golden["rec/" + case]).max())
        assert dp == float(golden["dp/" + case]) and force == float(golden["force/" + case])
        assert abs(R - float(golden["R/" + case])) <= 1e-9 * R
        found[case] = (dp, float(golden["R/" + case]))
    for pset, a, b in (("a15_k01", "a15_k01_r20", "a15_k01_r30"), ("a17_k10", "a17_k10_r20", "a17_k10_r28")):
        gamma = (found[a][0] - found[b][0]) / (1.0 / found[a][1] - 1.0 / found[b][1]) / 2.0
        print("%s %s: two-point Laplace slope / 2 = %.12g (oracle %.12g)" % (pset, schedule, gamma, float(golden["gamma/" + pset])))
        assert gamma == float(golden["gamma/" + pset])
    batch.close()
