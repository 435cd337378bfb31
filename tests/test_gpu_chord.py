"""GPU: chord traces (ChordTrace, bflbm_chord_*): the run-length distributions of a thresholded field along x, y and z,
recorded on the device as 64-bit integers.

The rule and the layout of a sample are in include/bflbm.h ("Chord traces"); analysis.chord_counts restates the rule in
numpy and tests/test_chord_abi.py holds it to a site-by-site walk, to the identities and to the closed forms.  Here the
device record is compared with chord_counts of the field the same lattice hands out, integer for integer: lone lattices of
both sources and both sides, 1 and 8 levels, max_length 4 (the last bin and long_sites in use) and 64, replicas of a
batch.  Every case asserts first, from the field and from what bflbm_chord_geometry reports, that the condition it is
there for really occurs."""
import ctypes

import numpy as np
import pytest

import chord_runs as cr
from test_gpu_morph import _batch_params, _field, _lattice, _schedule

pytestmark = pytest.mark.gpu

BOXES = {(7, 9, 5): "rows shorter than a wave, odd extents",
         (64, 3, 2): "a row exactly one wave block",
         (70, 5, 4): "a second block of 6 lanes, the 63|64 block boundary and the 69|0 seam",
         (130, 3, 2): "three blocks, the last of 2 lanes, room for a run that covers the whole middle block",
         (34, 31, 19): "y and z marches, line counts that are no multiple of 256",
         (6, 4, 1): "extent 1 along z, a row of 6",
         (2, 2, 2): "extent 2 along every axis"}
STATES = ["stripe", "noisy", "random", "planted"]
VARIABLES = {"hydrovs": "phi", "hydrovsbar": "rho"}
AXES = {"x": 2, "y": 1, "z": 0}                            # the array axis of field[nz][ny][nx]


def _levels8(x):
    """Eight levels from the finite values of x: one just below the least, six site values (the octiles of the distinct
    values: equality is hit; the median twice), one just above the greatest."""
    values = np.unique(x[np.isfinite(x)])
    big = np.finfo(np.float64).max
    below = max(float(np.nextafter(values[0], -np.inf)), -big)
    above = min(float(np.nextafter(values[-1], np.inf)), big)
    picks = [float(values[(len(values) * q) // 8]) for q in (1, 2, 4, 4, 6, 7)]
    return [below] + picks + [above]


def _lines(occ, axis):
    """The lines of a boolean set along an axis: [lines, n_a]."""
    return np.moveaxis(occ, AXES[axis], -1).reshape(-1, occ.shape[AXES[axis]])


def _assert_box(n, geo, nlevels, m, nrep=1):
    """What the box is there for, from the numbers the library reports."""
    assert geo == cr.geometry(n, nlevels, m, nrep)
    assert geo[2] == 1 + 3 * (3 + m) and geo[3] == nlevels * geo[2] <= cr.MAX_COUNTERS
    nx, ny, nz = n
    rows, gx, gy, gz = ny * nz, geo[4] // nrep, geo[5] // nrep, geo[6] // nrep
    assert gx == min(-(-rows // 4), max(1, cr.GROUPS // nrep)) and gy == -(-nx * nz // 256) and gz == -(-nx * ny // 256)
    if n == (7, 9, 5):
        assert nx < 64 and all(v % 2 for v in n) and rows % 4 == 1          # the last workgroup of the x launch has one row
    if n == (64, 3, 2):
        assert nx == 64
    if n == (70, 5, 4):
        assert nx // 64 == 1 and nx % 64 == 6
    if n == (130, 3, 2):
        assert nx // 64 == 2 and nx % 64 == 2
    if n == (34, 31, 19):
        assert (nx * nz) % 256 and (nx * ny) % 256 and gy == 3 and gz == 5 and ny > 8 and nz > 8 and ny % 8 and nz % 8
    if n == (6, 4, 1):
        assert nz == 1 and gz == 1
    if n == (2, 2, 2):
        assert n == (2, 2, 2) and (gx, gy, gz) == (1, 1, 1)


def _check(pkg, tr, x, levels, side, m, n):
    """One sample of a lone trace against the twin of x and the accessors against the record; returns record[nlevels, W]."""
    an = pkg.analysis
    tr.sample()
    steps, counts = tr.read()
    want = an.chord_counts(x, levels, side, m)
    assert counts.shape == (1, 1, len(levels), cr.words(m)) and counts.dtype == np.int64
    assert np.array_equal(counts[0, 0], want), (n, side, m, counts[0, 0, :, :8].tolist(), want[:, :8].tolist())
    layout = an.chord_blocks(m)
    assert np.array_equal(tr.occupied()[0, 0], want[:, 0])
    for name, na in zip("xyz", n):
        b = layout[name]
        assert np.array_equal(tr.chords(name)[0, 0], want[:, b["chords"]]) and np.array_equal(tr.spanning(name)[0, 0], want[:, b["spanning"]])
        h = tr.hist(name)[0, 0]
        assert np.array_equal(h, want[:, b["hist"]]) and np.array_equal(h.sum(axis=-1), want[:, b["chords"]])
        assert np.array_equal((np.arange(1, m) * h[:, :-1]).sum(axis=-1) + want[:, b["long_sites"]] + na * want[:, b["spanning"]], want[:, 0])
        mean, pdf = tr.mean_length(name)[0, 0], tr.pdf(name)[0, 0]
        for l in range(len(levels)):
            if want[l, b["chords"]]:
                assert mean[l] == (want[l, 0] - na * want[l, b["spanning"]]) / want[l, b["chords"]] and abs(pdf[l].sum() - 1.0) < 1e-12
            else:
                assert np.isnan(mean[l]) and np.isnan(pdf[l]).all()
    return counts[0, 0]


# ---- 1. a lone lattice against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,state", [(n, s) for n in BOXES for s in STATES])
def test_lone_record_equals_the_twin(pkg, n, state):
    lbm = _lattice(pkg, n, state)
    assert lbm.resolved_schedule() == _schedule(n)
    steps_done = lbm.steps_done
    sites = n[0] * n[1] * n[2]
    traces = []
    for source, name in VARIABLES.items():
        x = _field(pkg, lbm, source, name)
        eight = _levels8(x)
        for levels, m in ((eight, 4), (eight, 64), (eight[3:4], 4), (eight[3:4], 64)):
            for side in ("above", "below"):
                tr = lbm.chord_trace(name, levels, side=side, max_length=m, source=source, capacity=1)
                traces.append(tr)
                _assert_box(n, tr.geometry(), len(levels), m)
                rec = _check(pkg, tr, x, levels, side, m, n)
                assert tr.names == [name] and tr.read()[0].tolist() == [[steps_done]]
                layout = pkg.analysis.chord_blocks(m)
                if len(levels) == 8 and np.isfinite(x).all():
                    # below the least value: the whole torus, only spanning lines; above the greatest: nothing
                    whole, none = (0, 7) if side == "above" else (7, 0)
                    assert rec[whole, 0] == sites and not rec[none].any()
                    for axis, na in zip("xyz", n):
                        assert rec[whole, layout[axis]["chords"]] == 0 and rec[whole, layout[axis]["spanning"]] == sites // na
                    assert np.array_equal(rec[3], rec[4])                      # the median twice: the levels do not disturb each other
                if len(levels) == 8 and state == "random" and m == 4:
                    # scattered occupancy: chords of every short length along every axis longer than 5, the last bin in use,
                    # and, on the boxes with more than one wave block, runs across the block boundaries and across the seam in
                    # what the two sides record between them (six rows do not promise them to either side alone)
                    occs = [x >= t for t in levels[1:7]] + [x < t for t in levels[1:7]]
                    for axis, na in zip("xyz", n):
                        if na > 5 and sites // na >= 32:
                            assert (rec[1:7, layout[axis]["hist"]].sum(axis=0) > 0).all() and rec[1:7, layout[axis]["long_sites"]].sum() > 0
                    if n[0] > 64:
                        rows = [_lines(o, "x") for o in occs]
                        for edge in range(64, n[0], 64):
                            assert any((r[:, edge - 1] & r[:, edge]).any() for r in rows), edge
                        assert any((r[:, -1] & r[:, 0] & ~r.all(axis=1)).any() for r in rows)
                if state == "planted":                     # a NaN occupies nothing on either side
                    assert np.isnan(x).any()
    if state == "planted":                                 # both sides of one NaN-carrying field: the volumes do not add up to the box
        above, below = traces[0].occupied()[0, 0], traces[1].occupied()[0, 0]
        assert (above + below < sites).all()
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 2. the designed state: every seam and carry of the kernels, along each axis in turn -----------------------------------------
def _designed(n, axis):
    """(pattern[nz][ny][nx] of 0.1 / 1.0, the features placed): lines along `axis`, all other sites 0.1."""
    na = n["xyz".index(axis)]
    features = []
    if na >= 3:
        features.append(("seam", [na - 2, na - 1, 0] if na >= 4 else [na - 1, 0]))
    features.append(("full", list(range(na))))
    if na >= 2:
        features.append(("but one", [k for k in range(na) if k != na // 2]))
    if na > 65:
        features.append(("block boundary", list(range(60, min(68, na - 1)))))
    if na >= 130:
        features.append(("whole block", list(range(64, 128))))
    if na >= 3:
        features.append(("first site", [0]))
        features.append(("last site", [na - 1]))
    occ = np.zeros((n[2], n[1], n[0]), dtype=bool)
    lines = _lines(occ, axis).copy()                       # filled, then moved back
    if len(features) > len(lines) and na >= 130:           # (130, 3, 2) has six rows: the last site shares the whole block's line,
        features = [(w, s + [na - 1] if w == "whole block" else s) for w, s in features if w != "last site"]      # site 128 between them
        shared = ["last site"]
    else:
        shared = []
    placed = []
    step = max(1, len(lines) // len(features))
    for k, (what, where) in enumerate(features):
        if k * step < len(lines):
            lines[k * step, where] = True
            placed.append(what)
            placed += shared if what == "whole block" else []
    shape = list(occ.shape)
    shape.append(shape.pop(AXES[axis]))
    occ = np.moveaxis(lines.reshape(shape), -1, AXES[axis])
    return np.where(occ, 1.0, 0.1), placed


@pytest.mark.parametrize("n,axis", [(n, a) for n in BOXES for a in "xyz"])
def test_designed_state(pkg, n, axis):
    """Populations uploaded as pattern / 19, so that hydrovsbar rho is the 0.1 / 1.0 pattern; level 0.5."""
    pattern, placed = _designed(n, axis)
    na = n["xyz".index(axis)]
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=1.0, tau_f=1.0, tau_g=1.0), schedule=_schedule(n))
    lbm.LBM_init_mixture()
    f, g = lbm.populations()
    f[:] = pattern / 19.0
    g[:] = pattern / 19.0
    lbm.LBM_init(f, g)
    x = _field(pkg, lbm, "hydrovsbar", "rho")
    occ = x >= 0.5
    assert np.array_equal(occ, pattern > 0.5) and np.abs(x - pattern).max() < 1e-12
    lines = _lines(occ, axis)
    full, count = lines.all(axis=1), lines.sum(axis=1)
    assert "full" in placed and full.any()
    if "seam" in placed:
        assert (lines[:, 0] & lines[:, -1] & ~full).any()
    if "but one" in placed:
        assert (count == na - 1).any()
    if "block boundary" in placed:
        assert axis == "x" or na > 65
        assert (lines[:, 63] & lines[:, 64] & ~lines[:, 59] & ~full).any()
    if "whole block" in placed:
        assert (lines[:, 64:128].all(axis=1) & ~lines[:, 63] & ~lines[:, 128]).any()
    if "first site" in placed:                             # a chord of one site at either end of the line, on different lines
        assert (lines[:, 0] & ~lines[:, 1] & ~lines[:, -1]).any()
    if "last site" in placed:
        assert (lines[:, -1] & ~lines[:, -2] & ~lines[:, 0]).any()
    if n in ((70, 5, 4), (130, 3, 2)) and axis == "x":
        assert {"seam", "block boundary"} <= set(placed)
    if n == (130, 3, 2) and axis == "x":
        assert {"whole block", "first site", "last site"} <= set(placed)
    traces = []
    for m in (4, 64):
        for side in ("above", "below"):
            tr = lbm.chord_trace("rho", 0.5, side=side, max_length=m, source="hydrovsbar", capacity=1)
            traces.append(tr)
            _assert_box(n, tr.geometry(), 1, m)
            rec = _check(pkg, tr, x, [0.5], side, m, n)
            want = cr.record(occ if side == "above" else ~occ, m)                # the walk itself, not only the twin
            assert rec[0].tolist() == want
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 3. a batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,name,side,m", [("hydrovs", "phi", "above", 4), ("hydrovsbar", "rho", "below", 64)])
def test_batch_replicas_equal_the_twin_and_the_lattice_run_alone(pkg, source, name, side, m):
    n = (34, 31, 19)
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    batch.LBM_timestep(3)
    levels = _levels8(_field(pkg, batch.replicas[0], source, name))[2:5]          # one set of levels for all replicas
    tr = batch.chord_trace(name, levels, side=side, max_length=m, source=source, every=2, capacity=4)
    _assert_box(n, tr.geometry(), 3, m, nrep=3)
    tr.sample()
    steps, counts = tr.read()
    assert steps.tolist() == [[3, 1003, 3]] and counts.shape == (1, 3, 3, cr.words(m))
    for r, v in enumerate(batch.replicas):
        assert np.array_equal(counts[0, r], pkg.analysis.chord_counts(_field(pkg, v, source, name), levels, side, m)), (source, r)
    assert not np.array_equal(counts[0, 0], counts[0, 1]) and not np.array_equal(counts[0, 0], counts[0, 2])
    batch.LBM_timestep(4)                                  # samples after the batch steps 2 and 4
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == [3, 5, 7]
    assert tr.mean_length("z").shape == (3, 3, 3)
    batch.close()
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        if r == 1:
            lone.set_steps_done(1000)
        lone.LBM_timestep(3)
        alone = lone.chord_trace(name, levels, side=side, max_length=m, source=source, every=2, capacity=4)
        alone.sample()
        lone.LBM_timestep(4)
        a_steps, a_counts = alone.read()
        assert np.array_equal(a_steps[:, 0], steps[:, r]) and np.array_equal(a_counts[:, 0], counts[:, r]), (source, r)
        lone.close(); alone.close()
    assert np.array_equal(tr.read()[1], counts)            # detached, still readable
    tr.close()


# ---- 4. the morphology trace and the chord trace check each other ----------------------------------------------------------------
@pytest.mark.parametrize("side", ["above", "below"])
def test_interface_area_is_twice_the_chords_on_the_device_records(pkg, side):
    n = (13, 10, 6)
    lbm = _lattice(pkg, n, "noisy")
    levels = _levels8(_field(pkg, lbm, "hydrovs", "phi"))[1:7]
    mt = lbm.morphology_trace("phi", levels, side=side, every=1, capacity=8)
    ct = lbm.chord_trace("phi", levels, side=side, max_length=3, every=1, capacity=8)
    mt.sample(); ct.sample()
    lbm.LBM_timestep(5)
    f = mt.functionals()
    counts = mt.read()[1]
    assert f.shape[0] == 6 and ct.count == 6
    chords = ct.chords("x") + ct.chords("y") + ct.chords("z")
    assert np.array_equal(f[..., 1], 2 * chords) and np.array_equal(counts[..., 1] - 3 * counts[..., 0], chords)
    assert np.array_equal(ct.occupied(), counts[..., 0]) and (chords > 0).all()
    assert not np.array_equal(chords[0], chords[5])        # the state moved
    lbm.close(); mt.close(); ct.close()


# ---- 5. independence of what else is attached, of `every` and of the capacity ---------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders_every_or_capacity(pkg):
    n = (13, 10, 6)
    probe = _lattice(pkg, n, "noisy")
    levels = _levels8(_field(pkg, probe, "hydrovs", "phi"))[2:5]
    probe.close()
    records = {}
    for order in ("alone", "after the others"):
        lbm = _lattice(pkg, n, "noisy")
        others = []
        if order != "alone":
            others = [lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1), lbm.histogram_trace({"phi": (0.4, 0.6, 16)}, every=1, capacity=8),
                      lbm.spectrum_trace(["rho", "phi"], every=1, capacity=8), lbm.morphology_trace("phi", levels, every=1, capacity=8),
                      lbm.chord_trace("rho", levels, side="below", max_length=64, every=1, capacity=8)]
        tr = lbm.chord_trace("phi", levels, max_length=4, every=2 if order == "alone" else 1, capacity=3 if order == "alone" else 16)
        lbm.LBM_timestep(6)
        assert all(r.count == 6 for r in others)
        records[order] = tr.read()
        lbm.close(); tr.close()
    steps, counts = records["alone"]
    assert steps[:, 0].tolist() == [7, 9, 11] and not np.array_equal(counts[0], counts[2])
    steps2, counts2 = records["after the others"]
    assert steps2[:, 0].tolist() == [6, 7, 8, 9, 10, 11]
    assert np.array_equal(counts2[1::2], counts)


# ---- 6. the lifecycle -----------------------------------------------------------------------------------------------------------
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
    tr = o.chord_trace("rho", [0.999, 1.0, 1.001], max_length=4, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="chord trace full"):
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
    with pytest.raises(pkg.BflbmError, match="chord trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="chord trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, counts2 = tr.read()
    assert np.array_equal(counts, counts2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    w_steps, w_counts = tr.read(first=1, count=2)                         # a window of the record
    assert np.array_equal(w_counts, counts[1:]) and np.array_equal(w_steps, steps[1:])
    assert np.array_equal(tr.hist("y", first=1, count=2), tr.hist("y")[1:])
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


def test_chord_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lattice(pkg, (9, 7, 5), "noisy")
    lbm.set_steps_done(0)
    t = ctypes.c_void_p()
    levels = (ctypes.c_double * 2)(0.9995, 1.0005)
    check(lib.bflbm_chord_create(lbm._h, 1, 1, 2, levels, 1, 5, 1, 4, ctypes.byref(t)))     # hydrovsbar, component 1, below, M = 5
    lbm.LBM_timestep(3)
    as_ll = ctypes.POINTER(ctypes.c_longlong)
    w = cr.words(5)

    def read(first, count):
        counts, steps = np.empty((count, 1, 2, w), dtype=np.int64), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_chord_read(t, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return counts, steps
    counts0, steps0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3] and (counts0[..., 0] <= 315).all() and (counts0[:, 0, 0, 0] <= counts0[:, 0, 1, 0]).all()
    want = pkg.analysis.chord_counts(lbm.LBM_hydrovars_density()[1], [0.9995, 1.0005], "below", 5)
    assert np.array_equal(counts0[2, 0], want)
    geo = [ctypes.c_int() for _ in range(7)]
    check(lib.bflbm_chord_geometry(t, *[ctypes.byref(v) for v in geo]))
    assert tuple(v.value for v in geo) == cr.geometry((9, 7, 5), 2, 5)
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    counts1, steps1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(counts0, counts1)
    assert np.array_equal(read(2, 1)[0][0], counts0[2])    # a window
    assert lib.bflbm_chord_read(t, 2, 2, counts0.ctypes.data_as(as_ll), None) != 0
    assert lib.bflbm_chord_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_chord_destroy(t))


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm = _lattice(pkg, n, "noisy")
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_chord_create.*replica of a batch.*use bflbm_batch_chord_create"):
        batch.replicas[0].chord_trace("rho", [1.0])
    lib = pkg._lib.load()
    for owner, call in ((lbm, "bflbm_chord_create"), (batch, "bflbm_batch_chord_create")):
        nrep = 3 if owner is batch else 1
        # (pattern, source, var, levels, side, max_length, every, capacity), straight through the ABI: past the wrapper's own
        # checks; where two arguments are bad the header's order decides
        for pattern, source, var, levels, side, m, every, capacity in (
                ("1..8 levels \\(got 0\\)", 0, 0, [], 0, 64, 1, 4),
                ("1..8 levels \\(got 9\\)", 0, 0, [0.5] * 9, 0, 0, 1, 4),
                ("level 1 is not finite \\(got nan\\)", 0, 0, [0.5, np.nan], 0, 64, 1, 4),
                ("level 0 is not finite \\(got inf\\)", 0, 0, [np.inf], 0, 64, 1, 4),
                ("side must be 0 \\(v >= level\\) or 1 \\(v < level\\) \\(got 2\\)", 0, 0, [0.5], 2, 64, 1, 4),
                ("source must be 0 \\(hydrovs\\) or 1 \\(hydrovsbar\\) \\(got 2\\)", 2, 0, [0.5], 0, 64, 1, 4),
                ("variable index 22 outside hydrovs \\(0..21\\)", 0, 22, [0.5], 0, 0, 1, 4),
                ("variable index 9 outside hydrovsbar \\(0..8\\)", 1, 9, [0.5], 0, 64, 1, 4),
                ("max_length in 1..4096 \\(got 0\\)", 0, 0, [0.5], 0, 0, 0, 4),
                ("max_length in 1..4096 \\(got -1\\)", 0, 0, [0.5], 0, -1, 1, 4),
                ("max_length in 1..4096 \\(got 4097\\)", 0, 0, [0.5], 0, 4097, 1, 0),
                ("2 levels x 12298 words = 24596 counters per replica exceed 16384", 0, 0, [0.5, 0.6], 0, 4096, 0, 4),
                ("8 levels x 2050 words = 16400 counters per replica exceed 16384", 0, 0, [0.5] * 8, 0, 680, 1, 4),
                ("every must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 64, 0, 4),
                ("capacity must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 64, 1, 0),
                ("exceeds 1 TB", 0, 0, [0.5], 0, 64, 1, (1 << 37) // (202 * nrep) + 1)):
            h = ctypes.c_void_p()
            lv = (ctypes.c_double * max(len(levels), 1))(*levels)
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                pkg._lib.check(getattr(lib, call)(owner._h, source, var, len(levels), lv, side, m, every, capacity, ctypes.byref(h)))
            assert call in str(e.value) and not h.value, (call, str(e.value))
        h = ctypes.c_void_p()
        lv = (ctypes.c_double * 1)(0.5)
        for args in ((None, 0, 64, 1, 4, ctypes.byref(h)), (lv, 0, 64, 1, 4, None)):       # null pointers
            assert getattr(lib, call)(owner._h, 0, 0, 1, *args) != 0
            assert "null argument" in lib.bflbm_last_error().decode() and call in lib.bflbm_last_error().decode() and not h.value
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        # the limits themselves: the largest records, 64 KiB of LDS counters at the most, of the last component of either source
        for source, var, levels, m in (("hydrovs", 21, np.linspace(-1.0, 1.0, 8), 679), ("hydrovsbar", 8, [0.5], 4096)):
            full = owner.chord_trace(var, levels, max_length=m, source=source, capacity=1)
            full.sample()
            assert full.geometry()[:4] == (len(levels), m, cr.words(m), len(levels) * cr.words(m)) and full.geometry()[3] in (16376, 12298)
            rec = full.read()[1]
            assert rec.shape == (1, nrep, len(levels), cr.words(m))
            for r in range(nrep):
                view = owner.replicas[r] if owner is batch else owner
                assert np.array_equal(rec[0, r], pkg.analysis.chord_counts(_field(pkg, view, source, pkg.plotfile.variable_names(22 if source == "hydrovs" else 9)[var]), levels, "above", m))
            full.close()
    for bad in (lambda: lbm.chord_trace("no_such_variable", [1.0]), lambda: lbm.chord_trace(["rho", "phi"], [1.0]),
                lambda: lbm.chord_trace("rho", [1.0], side="left"), lambda: lbm.chord_trace("rho", [1.0], source="noise"),
                lambda: lbm.chord_trace("rho", [[1.0]])):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_chord_create inside an open step"):
        lbm.chord_trace("rho", [1.0])
    with pytest.raises(pkg.BflbmError, match="bflbm_chord_create inside an open step"):      # the open step comes before the cadence
        h = ctypes.c_void_p()
        pkg._lib.check(lib.bflbm_chord_create(lbm._h, 0, 0, 1, (ctypes.c_double * 1)(0.5), 0, 64, 0, 4, ctypes.byref(h)))
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.chord_trace("rho", [1.0], capacity=2)
    both = lbm.chord_trace("rho", [1.0], side="below", capacity=2)      # an owner carries several: both sides
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [6, 7]       # the split step samples in its finish
    assert both.count == 1 and tr.occupied()[1, 0, 0] + both.occupied()[0, 0, 0] == 512
    lbm.close(); batch.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_chord_create.*nranks > 1"):
        slab.chord_trace("rho", [1.0])
    slab.close()


# ---- 7. physics -----------------------------------------------------------------------------------------------------------------
def test_stripe_bands_are_the_z_chords(pkg):
    """A zero-noise stripe with the level between the phases: along z, nx ny chords per band, of that band's thickness;
    along x and y only spanning lines, thickness x ny and thickness x nx of them."""
    n = (12, 10, 24)
    lbm = _lattice(pkg, n, "stripe")
    x = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(x.max()) + float(x.min()))
    occ = x >= level
    column = occ[:, 0, 0]
    assert (occ == occ[:, :1, :1]).all() and 0 < column.sum() < n[2]
    spanning, bands = cr.line_runs([bool(v) for v in column])
    assert not spanning and len(bands) >= 1
    thickness = int(column.sum())
    m = 64
    tr = lbm.chord_trace("rho", level, max_length=m, capacity=1)
    tr.sample()
    assert tr.occupied()[0, 0, 0] == thickness * n[0] * n[1]
    hist = tr.hist("z")[0, 0, 0]
    want = np.zeros(m, dtype=np.int64)
    for b in bands:
        want[b - 1] += n[0] * n[1]
    assert np.array_equal(hist, want) and tr.chords("z")[0, 0, 0] == len(bands) * n[0] * n[1] and tr.spanning("z")[0, 0, 0] == 0
    assert tr.chords("x")[0, 0, 0] == 0 and tr.chords("y")[0, 0, 0] == 0
    assert tr.spanning("x")[0, 0, 0] == thickness * n[1] and tr.spanning("y")[0, 0, 0] == thickness * n[0]
    assert tr.mean_length("z")[0, 0, 0] == thickness / len(bands) and np.isnan(tr.mean_length("x")[0, 0, 0])
    lbm.close(); tr.close()


def test_spinodal_record_equals_the_twin_at_both_ends(pkg):
    """A 32^3 mixture at alpha0 = 2.5, kBT = 1e-5 sampled every 50 of 300 steps at the mean of phi: the first and the last
    sample equal the twin of the downloaded field.  The mean chords per axis are printed, not asserted: nobody has
    recorded them."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5, kBT=1e-5, seed=5), schedule="fused")
    lbm.LBM_init_mixture()
    level = float(_field(pkg, lbm, "hydrovs", "phi").mean())
    tr = lbm.chord_trace("phi", level, max_length=32, every=50, capacity=7)
    tr.sample()
    assert np.array_equal(tr.read()[1][0, 0], pkg.analysis.chord_counts(_field(pkg, lbm, "hydrovs", "phi"), [level], "above", 32))
    lbm.LBM_timestep(300)
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == [0, 50, 100, 150, 200, 250, 300]
    assert np.array_equal(counts[-1, 0], pkg.analysis.chord_counts(_field(pkg, lbm, "hydrovs", "phi"), [level], "above", 32))
    mean = [tr.mean_length(a)[:, 0, 0] for a in "xyz"]
    for k, step in enumerate(steps[:, 0]):
        print("spinodal step %4d: V = %6d  mean chord x %.3f  y %.3f  z %.3f" % (step, counts[k, 0, 0, 0], mean[0][k], mean[1][k], mean[2][k]))
    lbm.close(); tr.close()
