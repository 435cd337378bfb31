"""GPU: morphology traces (MorphologyTrace, bflbm_morph_*): the cubes, faces, edges and vertices of a thresholded field,
recorded on the device as 64-bit integers.

The counting rule and the layout of a sample are in include/bflbm.h ("Morphology traces"); analysis.minkowski_counts
restates the rule in numpy and tests/test_morph_abi.py holds it to a set construction and to the closed forms.  Here the
device record is compared with minkowski_counts of the field the same lattice hands out, integer for integer: lone
lattices of both sources and both sides, replicas of a batch.  The boxes are chosen from what bflbm_morph_geometry
reports, and every case asserts first that the condition it is there for really occurs.  The counting launch does not
stride: a work item is a workgroup, so there is no box with more work items than workgroups to test."""
import ctypes

import numpy as np
import pytest

import morph_counts as mc

pytestmark = pytest.mark.gpu

BOXES = {(7, 9, 5): "a plane below one tile, odd extents, one chunk, the two-pass schedule",
         (64, 32, 3): "two full tiles, fewer planes than the shortest chunk",
         (70, 30, 6): "three tiles, the last of 52 sites; rows of 70 wrap inside the tiles",
         (34, 31, 19): "two tiles, the last of 30 sites; chunks of 8, 8 and 3 planes: the hand-over and the z+ wrap of a short chunk"}
STATES = ["stripe", "noisy", "random", "planted"]
VARIABLES = {"hydrovs": ["rho", "phi", "ufy"], "hydrovsbar": ["phi", "rho", "ufx"]}


def _schedule(n):
    return "fused" if min(n) >= 5 and n != (7, 9, 5) else "two_pass"


def _lattice(pkg, n, state, **params):
    """stripe: a zero-noise stripe after 2 steps; noisy: a mixture at kBT = 1e-5 after 5 steps; random: populations drawn
    site by site and uploaded, so that every field is scattered about its median; planted: the noisy state uploaded again
    with NaN and huge populations at four sites (the histogram tests' state)."""
    p = dict(kBT=0.0 if state == "stripe" else 1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0, seed=77)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=_schedule(n))
    if state == "stripe":
        lbm.LBM_init_stripe(0.5)
        lbm.LBM_timestep(2)
        return lbm
    lbm.LBM_init_mixture()
    lbm.LBM_timestep(5)
    if state == "random":
        f, g = lbm.populations()
        rng = np.random.default_rng(n[0] + 100 * n[1] + 10000 * n[2])
        lbm.LBM_init(rng.uniform(0.01, 0.1, size=f.shape), rng.uniform(0.01, 0.1, size=g.shape))
    if state == "planted":
        f, g = lbm.populations()
        flat_f, flat_g = f.reshape(f.shape[0], -1), g.reshape(g.shape[0], -1)
        sites = flat_f.shape[1]
        flat_f[:, sites // 3] = np.nan
        flat_g[3, sites // 2] = np.nan
        flat_f[0, sites - 1] = 1e200
        flat_g[0, 0] = -1e200
        lbm.LBM_init(f, g)
    return lbm


def _field(pkg, lat, source, name):
    """One variable of the resident state through the full-field getters: [nz][ny][nx]."""
    full = lat.LBM_hydrovars() if source == "hydrovs" else lat.LBM_hydrovars_density()
    return full[pkg.plotfile.variable_names(22 if source == "hydrovs" else 9).index(name)].copy()


def _levels(x):
    """Five levels from the finite values of x: one just below the least, three that are site values (the quartiles of the
    distinct values: equality is hit), one just above the greatest."""
    values = np.unique(x[np.isfinite(x)])
    big = np.finfo(np.float64).max
    below = max(float(np.nextafter(values[0], -np.inf)), -big)
    above = min(float(np.nextafter(values[-1], np.inf)), big)
    picks = [float(values[(len(values) * q) // 4]) for q in (1, 2, 3)]
    return [below] + picks + [above]


def _assert_geometry(n, geo, nlevels, nrep=1):
    """What the box is there for, from the numbers the library reports."""
    assert geo == mc.geometry(n, nlevels, nrep)
    _, tile, zc, items, groups = geo
    plane, nz = n[0] * n[1], n[2]
    tiles, chunks = -(-plane // tile), -(-nz // zc)
    assert items == tiles * chunks and groups == items * nrep                  # no stride: a workgroup per work item
    if n == (7, 9, 5):
        assert plane < tile and chunks == 1 and zc == nz and all(v % 2 for v in n)
    if n == (64, 32, 3):
        assert plane == 2 * tile and chunks == 1 and zc == nz < mc.MIN_CHUNK
    if n == (70, 30, 6):
        assert tiles == 3 and 0 < plane % tile < tile and tile % n[0] != 0 and chunks == 1
    if n == (34, 31, 19):
        assert tiles == 2 and plane % tile == 30 and chunks == 3 and nz % zc == 3


# ---- 1. a lone lattice against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,state", [(n, s) for n in BOXES for s in STATES])
def test_lone_record_equals_the_twin(pkg, n, state):
    lbm = _lattice(pkg, n, state)
    assert lbm.resolved_schedule() == _schedule(n)
    steps_done = lbm.steps_done
    sites = n[0] * n[1] * n[2]
    traces = []
    for source, names in VARIABLES.items():
        for name in names:
            x = _field(pkg, lbm, source, name)
            levels = _levels(x)
            for side in ("above", "below"):
                tr = lbm.morphology_trace(name, levels, side=side, source=source, capacity=1)
                traces.append(tr)
                _assert_geometry(n, tr.geometry(), 5)
                tr.sample()
                steps, counts = tr.read()
                want = pkg.analysis.minkowski_counts(x, levels, side)          # the getters leave the resident state as it is
                assert counts.shape == (1, 1, 5, 4) and counts.dtype == np.int64 and steps.tolist() == [[steps_done]]
                assert np.array_equal(counts[0, 0], want), (n, state, source, name, side, counts[0, 0].tolist(), want.tolist())
                assert tr.names == [name] and np.array_equal(tr.functionals()[0, 0], pkg.analysis.minkowski_functionals(want))
                whole, none = [sites, 3 * sites, 3 * sites, sites], [0, 0, 0, 0]
                if np.isfinite(x).all():                   # below the least value: the whole torus; above the greatest: nothing
                    assert counts[0, 0, 0].tolist() == (whole if side == "above" else none)
                    assert counts[0, 0, 4].tolist() == (none if side == "above" else whole)
                    for l in (1, 2, 3):                    # the level is a site value: that site is occupied above, not below
                        assert counts[0, 0, l, 0] == np.count_nonzero(x >= levels[l] if side == "above" else x < levels[l])
                        assert np.count_nonzero(x == levels[l]) >= 1
                elif name in ("rho", "phi"):               # a NaN occupies nothing on either side: the two volumes miss it
                    assert state == "planted" and np.isnan(x).any()
                if state == "random" and name in ("rho", "phi"):       # scattered occupancy near one half: what finds a wrong neighbour
                    assert 0.4 * sites < counts[0, 0, 2, 0] < 0.6 * sites and counts[0, 0, 2, 3] > counts[0, 0, 2, 0]
    if state == "planted":                                 # both sides of one NaN-carrying field: the volumes do not add up to the box
        above, below = traces[0].read()[1][0, 0], traces[1].read()[1][0, 0]
        assert (above[:, 0] + below[:, 0] < sites).all()
    if state == "stripe":                                  # planes of one phase: chi = 0 and S = 2 nx ny per pair of interfaces
        x = _field(pkg, lbm, "hydrovs", "rho")
        level = 0.5 * (float(x.max()) + float(x.min()))
        occ = x >= level
        assert (occ == occ[:, :1, :1]).all() and 0 < occ[:, 0, 0].sum() < n[2]
        runs = int(np.count_nonzero(occ[:, 0, 0] & ~np.roll(occ[:, 0, 0], 1)))
        tr = lbm.morphology_trace("rho", level, capacity=1)
        traces.append(tr)
        tr.sample()
        v, s, b2, chi = tr.functionals()[0, 0, 0].tolist()
        assert (v, s, b2, chi) == (int(occ.sum()), 2 * n[0] * n[1] * runs, 0, 0) and runs >= 1
        assert tr.length()[0, 0, 0] == sites / s
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 2. a batch -----------------------------------------------------------------------------------------------------------------
def _batch_params():
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


@pytest.mark.parametrize("source,name,side", [("hydrovs", "phi", "above"), ("hydrovsbar", "rho", "below"), ("hydrovs", "ufz", "above")])
def test_batch_replicas_equal_the_twin_and_the_lattice_run_alone(pkg, source, name, side):
    n = (34, 31, 19)
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    batch.LBM_timestep(3)
    levels = _levels(_field(pkg, batch.replicas[0], source, name))[1:4]          # one set of levels for all replicas
    tr = batch.morphology_trace(name, levels, side=side, source=source, every=2, capacity=4)
    _assert_geometry(n, tr.geometry(), 3, nrep=3)
    tr.sample()
    steps, counts = tr.read()
    assert steps.tolist() == [[3, 1003, 3]] and counts.shape == (1, 3, 3, 4)
    for r, v in enumerate(batch.replicas):
        assert np.array_equal(counts[0, r], pkg.analysis.minkowski_counts(_field(pkg, v, source, name), levels, side)), (source, r)
    assert not np.array_equal(counts[0, 0], counts[0, 1]) and not np.array_equal(counts[0, 0], counts[0, 2])
    batch.LBM_timestep(4)                                  # samples after the batch steps 2 and 4
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == [3, 5, 7]
    batch.close()
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        if r == 1:
            lone.set_steps_done(1000)
        lone.LBM_timestep(3)
        alone = lone.morphology_trace(name, levels, side=side, source=source, every=2, capacity=4)
        alone.sample()
        lone.LBM_timestep(4)
        a_steps, a_counts = alone.read()
        assert np.array_equal(a_steps[:, 0], steps[:, r]) and np.array_equal(a_counts[:, 0], counts[:, r]), (source, r)
        lone.close(); alone.close()
    assert np.array_equal(tr.read()[1], counts)            # detached, still readable
    tr.close()


# ---- 3. independence of what else is attached, of `every` and of the capacity ---------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders_every_or_capacity(pkg):
    n = (13, 10, 6)
    probe = _lattice(pkg, n, "noisy")
    levels = _levels(_field(pkg, probe, "hydrovs", "phi"))[1:4]
    probe.close()
    records = {}
    for order in ("alone", "after the others"):
        lbm = _lattice(pkg, n, "noisy")
        others = []
        if order != "alone":
            others = [lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1), lbm.histogram_trace({"phi": (0.4, 0.6, 16)}, every=1, capacity=8),
                      lbm.spectrum_trace(["rho", "phi"], every=1, capacity=8), lbm.profile_trace(["rho", "afz"], [("rho", "afz")], axis="y", every=1, capacity=8),
                      lbm.morphology_trace("rho", levels, side="below", every=1, capacity=8)]
        tr = lbm.morphology_trace("phi", levels, every=2 if order == "alone" else 1, capacity=3 if order == "alone" else 16)
        lbm.LBM_timestep(6)
        assert all(r.count == 6 for r in others)
        records[order] = tr.read()
        lbm.close(); tr.close()
    steps, counts = records["alone"]
    assert steps[:, 0].tolist() == [7, 9, 11] and not np.array_equal(counts[0], counts[2])
    steps2, counts2 = records["after the others"]
    assert steps2[:, 0].tolist() == [6, 7, 8, 9, 10, 11]
    assert np.array_equal(counts2[1::2], counts)


# ---- 4. the lifecycle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n = (9, 7, 5)
    if owner == "lone":
        o = _lattice(pkg, n, "noisy")
        o.set_steps_done(0)
    else:
        o = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
        for v in o.replicas:
            v.LBM_init_mixture()
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: o.replicas[0].steps_done)
    other = o.trace(every=1, capacity=16)
    tr = o.morphology_trace("rho", [0.999, 1.0, 1.001], every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="morphology trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    assert tr.count == 1 and tr.read()[0][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    steps, counts = tr.read()
    with pytest.raises(pkg.BflbmError, match="morphology trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="morphology trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, counts2 = tr.read()
    assert np.array_equal(counts, counts2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    w_steps, w_counts = tr.read(first=1, count=2)                         # a window of the record
    assert np.array_equal(w_counts, counts[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[0][0, 0] == 7
    # the owner goes first: the trace stays readable with the same integers, refuses a sample, closes twice
    steps, counts = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, counts2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(counts, counts2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_morphology_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lattice(pkg, (9, 7, 5), "noisy")
    lbm.set_steps_done(0)
    t = ctypes.c_void_p()
    levels = (ctypes.c_double * 2)(0.9995, 1.0005)
    check(lib.bflbm_morph_create(lbm._h, 1, 1, 2, levels, 1, 1, 4, ctypes.byref(t)))     # hydrovsbar, component 1, below
    lbm.LBM_timestep(3)
    as_ll = ctypes.POINTER(ctypes.c_longlong)

    def read(first, count):
        counts, steps = np.empty((count, 1, 2, 4), dtype=np.int64), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_morph_read(t, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return counts, steps
    counts0, steps0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3] and (counts0[..., 0] <= 315).all() and (counts0[:, 0, 0] <= counts0[:, 0, 1]).all()
    want = pkg.analysis.minkowski_counts(lbm.LBM_hydrovars_density()[1], [0.9995, 1.0005], "below")
    assert np.array_equal(counts0[2, 0], want)
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    counts1, steps1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(counts0, counts1)
    assert np.array_equal(read(2, 1)[0][0], counts0[2])    # a window
    assert lib.bflbm_morph_read(t, 2, 2, counts0.ctypes.data_as(as_ll), None) != 0
    assert lib.bflbm_morph_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_morph_destroy(t))


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm = _lattice(pkg, n, "noisy")
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_morph_create.*replica of a batch.*use bflbm_batch_morph_create"):
        batch.replicas[0].morphology_trace("rho", [1.0])
    lib = pkg._lib.load()
    for owner, call in ((lbm, "bflbm_morph_create"), (batch, "bflbm_batch_morph_create")):
        nrep = 3 if owner is batch else 1
        # (pattern, source, var, levels, side, every, capacity), straight through the ABI: past the wrapper's own checks
        for pattern, source, var, levels, side, every, capacity in (
                ("1..8 levels \\(got 0\\)", 0, 0, [], 0, 1, 4),
                ("1..8 levels \\(got 9\\)", 0, 0, [0.5] * 9, 0, 1, 4),
                ("level 1 is not finite \\(got nan\\)", 0, 0, [0.5, np.nan], 0, 1, 4),
                ("level 0 is not finite \\(got inf\\)", 0, 0, [np.inf], 0, 1, 4),
                ("level 2 is not finite \\(got -inf\\)", 0, 0, [0.0, 1.0, -np.inf], 0, 1, 4),
                ("side must be 0 \\(v >= level\\) or 1 \\(v < level\\) \\(got 2\\)", 0, 0, [0.5], 2, 1, 4),
                ("side must be 0 .* \\(got -1\\)", 0, 0, [0.5], -1, 1, 4),
                ("source must be 0 \\(hydrovs\\) or 1 \\(hydrovsbar\\) \\(got 2\\)", 2, 0, [0.5], 0, 1, 4),
                ("source must be 0 .* \\(got -1\\)", -1, 0, [0.5], 0, 1, 4),
                ("variable index 22 outside hydrovs \\(0..21\\)", 0, 22, [0.5], 0, 1, 4),
                ("variable index -1 outside hydrovs", 0, -1, [0.5], 0, 1, 4),
                ("variable index 9 outside hydrovsbar \\(0..8\\)", 1, 9, [0.5], 0, 1, 4),
                ("every must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 0, 4),
                ("capacity must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 1, 0),
                ("exceeds 1 TB", 0, 0, [0.5], 0, 1, (1 << 37) // (4 * nrep) + 1)):
            h = ctypes.c_void_p()
            lv = (ctypes.c_double * max(len(levels), 1))(*levels)
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                pkg._lib.check(getattr(lib, call)(owner._h, source, var, len(levels), lv, side, every, capacity, ctypes.byref(h)))
            assert call in str(e.value) and not h.value, (call, str(e.value))
        h = ctypes.c_void_p()
        lv = (ctypes.c_double * 1)(0.5)
        for args in ((None, 0, 1, 4, ctypes.byref(h)), (lv, 0, 1, 4, None)):       # null pointers
            assert getattr(lib, call)(owner._h, 0, 0, 1, *args) != 0
            assert "null argument" in lib.bflbm_last_error().decode() and call in lib.bflbm_last_error().decode() and not h.value
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        # the limits themselves: 8 levels of the last component of either source
        for source, var in (("hydrovs", 21), ("hydrovsbar", 8)):
            full = owner.morphology_trace(var, np.linspace(-1.0, 1.0, 8), source=source, capacity=1)
            full.sample()
            assert full.geometry()[0] == 8 and full.read()[1].shape == (1, nrep, 8, 4)
            full.close()
    for bad in (lambda: lbm.morphology_trace("no_such_variable", [1.0]), lambda: lbm.morphology_trace(["rho", "phi"], [1.0]),
                lambda: lbm.morphology_trace("rho", [1.0], side="left"), lambda: lbm.morphology_trace("rho", [1.0], source="noise"),
                lambda: lbm.morphology_trace("rho", [[1.0]])):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_morph_create inside an open step"):
        lbm.morphology_trace("rho", [1.0])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.morphology_trace("rho", [1.0], capacity=2)
    both = lbm.morphology_trace("rho", [1.0], side="below", capacity=2)      # an owner carries several: both sides
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [6, 7]       # the split step samples in its finish
    assert both.count == 1 and tr.read()[1][1, 0, 0, 0] + both.read()[1][0, 0, 0, 0] == 512
    lbm.close(); batch.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_morph_create.*nranks > 1"):
        slab.morphology_trace("rho", [1.0])
    slab.close()


# ---- 5. physics -----------------------------------------------------------------------------------------------------------------
def test_droplet_is_one_component_and_its_area_is_twice_its_projections(pkg):
    """A 32^3 droplet after 5 zero-noise steps at the level midway between the extremes of its rho: chi = 1, and, the
    mask being orthogonally convex (asserted first), S = 2 x the three projected areas of the downloaded mask."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=2.5), schedule="fused")
    lbm.LBM_init_droplet(0.3)
    lbm.LBM_timestep(5)
    rho = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(rho.max()) + float(rho.min()))
    mask = rho >= level
    assert mc.orthogonally_convex(mask) and 0 < mask.sum() < mask.size
    assert not (mask[0].any() or mask[:, 0].any() or mask[:, :, 0].any())          # away from the periodic planes
    tr = lbm.morphology_trace("rho", level, capacity=1)
    _assert_geometry(n, tr.geometry(), 1)
    tr.sample()
    v, s, b2, chi = tr.functionals()[0, 0, 0].tolist()
    print("droplet: V = %d, S = %d, 2B = %d, chi = %d, projections %s" % (v, s, b2, chi, mc.projections(mask)))
    assert chi == 1 and v == int(mask.sum()) and s == 2 * sum(mc.projections(mask))
    lbm.close(); tr.close()


def test_spinodal_record_equals_the_twin_at_both_ends(pkg):
    """A 32^3 mixture at alpha0 = 2.5, kBT = 1e-5 sampled every 50 of 300 steps at the mean of phi: the first and the
    last sample equal the twin of the downloaded field.  chi(t) and L(t) = nsites / S are printed, not asserted: nobody
    has recorded them."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5, kBT=1e-5, seed=5), schedule="fused")
    lbm.LBM_init_mixture()
    level = float(_field(pkg, lbm, "hydrovs", "phi").mean())
    tr = lbm.morphology_trace("phi", level, every=50, capacity=7)
    tr.sample()
    assert np.array_equal(tr.read()[1][0, 0], pkg.analysis.minkowski_counts(_field(pkg, lbm, "hydrovs", "phi"), [level]))
    lbm.LBM_timestep(300)
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == [0, 50, 100, 150, 200, 250, 300]
    assert np.array_equal(counts[-1, 0], pkg.analysis.minkowski_counts(_field(pkg, lbm, "hydrovs", "phi"), [level]))
    f, length = tr.functionals(), tr.length()
    for k, step in enumerate(steps[:, 0]):
        print("spinodal step %4d: V = %6d  S = %6d  chi = %6d  L = %.3f" % (step, f[k, 0, 0, 0], f[k, 0, 0, 1], f[k, 0, 0, 3], length[k, 0, 0]))
    lbm.close(); tr.close()
