"""GPU: cluster traces (ClusterTrace, bflbm_cluster_*): the connected components of a thresholded field, labelled on the
device by a union-find and recorded as 64-bit integers.

The definition and the layout of a sample are in include/bflbm.h ("Cluster traces"); analysis.cluster_record and
analysis.cluster_labels restate the rule in numpy and tests/test_cluster_abi.py holds them to a flood fill and to the
closed forms.  Here the device record and the device labels are compared with the twin of the field the same lattice hands
out, integer for integer: lone lattices of both sources, both sides and both connectivities, replicas of a batch, planted
sets.  The boxes are chosen from what bflbm_cluster_geometry reports, and every case asserts first, from the geometry and
from the twin's labels of the downloaded field, that the condition it is there for really occurs.  Word 5 (capped) is only
ever asserted to be zero: no test provokes the cap."""
import ctypes

import numpy as np
import pytest

import cluster_sets as cs
from test_gpu_morph import _batch_params, _field, _lattice, _schedule

pytestmark = pytest.mark.gpu

BOXES = {(7, 3, 3): "smaller than a brick in every direction, odd extents: one brick whose every wrapped link is its own",
         (7, 9, 5): "odd extents, ragged bricks along y and z, the two-pass schedule",
         (32, 6, 5): "the x extent is the brick's: a wrapped link along x joins a brick to itself",
         (70, 30, 6): "a ragged last brick along every axis: 70 = 2 x 32 + 6, 30 = 7 x 4 + 2, 6 = 4 + 2",
         (34, 31, 19): "a ragged last brick along every axis, 80 bricks",
         (2, 2, 2): "the + and - neighbours coincide along every axis",
         (1, 3, 2): "a site is its own neighbour along x"}
STATES = ["stripe", "noisy", "random", "planted"]
FILLS = [0.05, 0.10, 0.31, 0.5, 0.9]     # 0.10 and 0.31: near the site-percolation thresholds of the 26- and 6-neighbour lattices
VARIABLES = {"hydrovs": "phi", "hydrovsbar": "rho"}


def _levels(x, side):
    """Five levels that are site values (equality is hit), at which the occupied fraction of the finite sites is about
    FILLS on the given side."""
    values = np.sort(x[np.isfinite(x)].ravel())
    qs = FILLS if side == "below" else [1.0 - q for q in FILLS]
    return [float(values[min(int(q * len(values)), len(values) - 1)]) for q in qs]


def _assert_geometry(n, geo, nlevels, connectivity):
    """What the box is there for, from the numbers the library reports."""
    assert geo == cs.geometry(n, nlevels, connectivity)
    bx, by, bz = geo[2:5]
    assert geo[5] == -(-n[0] // bx) * -(-n[1] // by) * -(-n[2] // bz)
    if n == (7, 3, 3):
        assert n[0] < bx and n[1] < by and n[2] < bz and geo[5] == 1 and all(v % 2 for v in n)
    if n == (32, 6, 5):
        assert n[0] == bx
    if n in ((70, 30, 6), (34, 31, 19)):
        assert n[0] % bx and n[1] % by and n[2] % bz and geo[5] > 1
    if n == (34, 31, 19):
        assert geo[5] == 80


def _assert_identities(rec, sites):
    """What holds for every record: rec[..., 38]."""
    rec = np.asarray(rec).reshape(-1, cs.WORDS)
    for r in rec.tolist():
        ncomp, vol, smax, label, s2, capped = r[:6]
        assert capped == 0 and sum(r[6:]) == ncomp and 0 <= ncomp <= vol <= sites
        assert smax * smax <= s2 <= vol * vol and (label == -1) == (ncomp == 0) == (smax == 0) and -1 <= label < sites


def _check(pkg, tr, x, levels, side, connectivity, all_labels=True):
    """One sample and the labels of a lone trace against the twin of x; returns (record[nlevels, 38], twin labels)."""
    an = pkg.analysis
    tr.sample()
    steps, rec = tr.read()
    want = an.cluster_record(x, levels, side, connectivity)
    assert rec.shape == (1, 1, len(levels), cs.WORDS) and rec.dtype == np.int64
    assert np.array_equal(rec[0, 0], want), (side, connectivity, rec[0, 0, :, :6].tolist(), want[:, :6].tolist())
    _assert_identities(rec, x.size)
    twins = {}
    for l in (range(len(levels)) if all_labels else [2]):
        twins[l] = an.cluster_labels(x, levels[l], side, connectivity)
        got = tr.labels(l)
        assert got.shape == (1,) + x.shape and got.dtype == np.int32
        assert np.array_equal(got[0], twins[l]), (side, connectivity, l)
        roots, sizes = an.cluster_sizes(got[0])
        assert len(roots) == rec[0, 0, l, 0] and (sizes.max() if len(sizes) else 0) == rec[0, 0, l, 2]
        if len(roots):
            assert rec[0, 0, l, 3] == roots[sizes == sizes.max()].min()      # word 3: the smallest label of the largest size
    assert tr.count == 1                                   # labels() records nothing
    assert np.array_equal(tr.read()[1], rec)               # and leaves the totals as they are: the sample reads the same
    return rec[0, 0], twins


# ---- 1. a lone lattice against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,state", [(n, s) for n in BOXES for s in STATES])
def test_lone_record_and_labels_equal_the_twin(pkg, n, state):
    lbm = _lattice(pkg, n, state)
    steps_done = lbm.steps_done
    sites = n[0] * n[1] * n[2]
    traces = []
    for source, name in VARIABLES.items():
        x = _field(pkg, lbm, source, name)
        for side in ("above", "below"):
            levels = _levels(x, side)
            mt = lbm.morphology_trace(name, levels, side=side, source=source, capacity=1)
            mt.sample()
            volumes = mt.read()[1][0, 0, :, 0]
            traces.append(mt)
            for connectivity in cs.CONNECTIVITIES:
                tr = lbm.cluster_trace(name, levels, side=side, connectivity=connectivity, source=source, capacity=2)
                traces.append(tr)
                _assert_geometry(n, tr.geometry(), 5, connectivity)
                rec, twins = _check(pkg, tr, x, levels, side, connectivity, all_labels=source == "hydrovs")
                assert tr.read()[0].tolist() == [[steps_done]] and tr.names == [name]
                assert np.array_equal(rec[:, 1], volumes)                      # word 1 is the morphology trace's N3
                assert np.array_equal(tr.components()[0, 0], rec[:, 0]) and np.array_equal(tr.size_histogram()[0, 0], rec[:, 6:])
                assert np.array_equal(tr.largest()[0][0, 0], rec[:, 2]) and np.array_equal(tr.largest()[1][0, 0], rec[:, 3])
                number, weight = tr.mean_sizes()
                for l in range(5):
                    if rec[l, 0]:
                        assert number[0, 0, l] == rec[l, 1] / rec[l, 0] and weight[0, 0, l] == rec[l, 4] / rec[l, 1]
                if state == "random" and source == "hydrovs" and n in ((34, 31, 19), (70, 30, 6)):
                    frac = rec[:, 1] / sites                                    # the fills are what the levels were chosen for
                    assert np.allclose(frac, FILLS, atol=0.01), frac
                    if connectivity == 6:
                        assert rec[0, 0] > 100 and rec[1, 0] > 100             # many small components below the threshold
                    for l in (2, 3, 4):                                         # fills >= 0.31: components across bricks and wraps
                        lab = twins[l]
                        roots, sizes = pkg.analysis.cluster_sizes(lab)
                        largest = roots[np.argsort(-sizes, kind="stable")[:5]].tolist()
                        assert int(rec[l, 3]) == largest[0] and len(cs.bricks_of(lab, largest[0])) >= 2
                        assert any(cs.wrapped_axes(lab, big, connectivity) == {0, 1, 2} for big in largest)
                    assert rec[4, 2] > 0.95 * rec[4, 1]                         # at 0.9 one component holds nearly every site
    if state == "planted":                                 # a NaN occupies nothing on either side
        x = _field(pkg, lbm, "hydrovs", "phi")
        assert np.isnan(x).any()
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 2. planted sets ------------------------------------------------------------------------------------------------------------
def _planted(pkg, n, mask):
    """A lattice whose rho takes one of two values by the mask[nz, ny, nx]: populations uploaded, f by the mask, g constant."""
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=1.0, tau_f=1.0, tau_g=1.0), schedule=_schedule(n))
    lbm.LBM_init_mixture()
    f, g = lbm.populations()
    assert f.shape[1:] == mask.shape
    f[:] = np.where(mask, 0.05, 0.02)
    g[:] = 0.03
    lbm.LBM_init(f, g)
    return lbm


def _sets(n):
    nx, ny, nz = n
    z, y, x = np.indices((nz, ny, nx))
    out = {"snake": cs.snake((nz, ny, nx)), "checkerboard": (z + y + x) % 2 == 0, "full": np.ones((nz, ny, nx), dtype=bool),
           "empty": np.zeros((nz, ny, nx), dtype=bool)}
    slabs = np.zeros((nz, ny, nx), dtype=bool)
    slabs[[nz - 1, 0]] = True                             # across the periodic plane
    slabs[nz // 2] = True
    out["slabs"] = slabs
    stairs = np.zeros((nz, ny, nx), dtype=bool)
    for i in range(min(n) - 1):                            # corner-touching voxels, clear of the periodic planes
        stairs[i, i, i] = True
    out["staircase"] = stairs
    return out


@pytest.mark.parametrize("n", [(34, 31, 19), (32, 6, 6)])
@pytest.mark.parametrize("which", ["snake", "checkerboard", "full", "empty", "slabs", "staircase"])
def test_planted_sets_equal_their_closed_forms_and_the_twin(pkg, n, which):
    mask = _sets(n)[which]
    sites = mask.size
    lbm = _planted(pkg, n, mask)
    x = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(x.max()) + float(x.min())) if which not in ("full", "empty") else (0.5 if which == "full" else 2.0)
    assert np.array_equal(x >= level, mask)                # the set on the device is the set that was planted
    traces = []
    for connectivity in cs.CONNECTIVITIES:
        tr = lbm.cluster_trace("rho", level, connectivity=connectivity, capacity=1)
        traces.append(tr)
        rec, twins = _check(pkg, tr, x, [level], "above", connectivity)
        r = rec[0].tolist()
        v = int(mask.sum())
        if which == "snake":                               # one component through every brick, its label its far end
            assert r[:5] == [1, v, v, 0, v * v] and v > sites // 8
            assert len(cs.bricks_of(twins[0], 0)) == tr.geometry()[5] > 1
        if which == "checkerboard":
            even = all(e % 2 == 0 for e in n)
            if connectivity == 6 and even:
                assert r[:5] == [sites // 2, sites // 2, 1, 0, sites // 2] and r[6] == sites // 2
            if connectivity == 26:
                assert r[:4] == [1, v, v, 0]
        if which == "full":
            assert r[:5] == [1, sites, sites, 0, sites * sites] and r[6 + sites.bit_length() - 1] == 1
        if which == "empty":
            assert r == [0, 0, 0, -1] + [0] * 34 and (twins[0] == -1).all()
        if which == "slabs":
            plane = n[0] * n[1]
            assert r[:5] == [2, 3 * plane, 2 * plane, 0, 5 * plane * plane]
            assert (twins[0][[n[2] - 1, 0]] == 0).all() and (twins[0][n[2] // 2] == (n[2] // 2) * plane).all()
        if which == "staircase":
            k = min(n) - 1
            assert r[:5] == ([1, k, k, 0, k * k] if connectivity == 26 else [k, k, 1, 0, k])
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 3. a batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,name,side,connectivity", [("hydrovs", "phi", "above", 26), ("hydrovsbar", "rho", "below", 6)])
def test_batch_replicas_equal_the_twin_and_the_lattice_run_alone(pkg, source, name, side, connectivity):
    n = (34, 31, 19)
    an = pkg.analysis
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    batch.LBM_timestep(3)
    levels = _levels(_field(pkg, batch.replicas[0], source, name), side)[1:4]          # one set of levels for all replicas
    tr = batch.cluster_trace(name, levels, side=side, connectivity=connectivity, source=source, every=2, capacity=4)
    assert tr.geometry() == cs.geometry(n, 3, connectivity)
    tr.sample()
    steps, rec = tr.read()
    assert steps.tolist() == [[3, 1003, 3]] and rec.shape == (1, 3, 3, cs.WORDS)
    _assert_identities(rec, n[0] * n[1] * n[2])
    labels = [tr.labels(l) for l in range(3)]
    for r, v in enumerate(batch.replicas):
        x = _field(pkg, v, source, name)
        assert np.array_equal(rec[0, r], an.cluster_record(x, levels, side, connectivity)), (source, r)
        for l in range(3):
            assert np.array_equal(labels[l][r], an.cluster_labels(x, levels[l], side, connectivity)), (source, r, l)
    assert not np.array_equal(rec[0, 0], rec[0, 1]) and not np.array_equal(rec[0, 0], rec[0, 2])
    assert not np.array_equal(labels[1][0], labels[1][1])
    batch.LBM_timestep(4)                                  # samples after the batch steps 2 and 4
    steps, rec = tr.read()
    assert steps[:, 0].tolist() == [3, 5, 7]
    batch.close()
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        if r == 1:
            lone.set_steps_done(1000)
        lone.LBM_timestep(3)
        alone = lone.cluster_trace(name, levels, side=side, connectivity=connectivity, source=source, every=2, capacity=4)
        alone.sample()
        assert np.array_equal(alone.labels(1)[0], labels[1][r])
        lone.LBM_timestep(4)
        a_steps, a_rec = alone.read()
        assert np.array_equal(a_steps[:, 0], steps[:, r]) and np.array_equal(a_rec[:, 0], rec[:, r]), (source, r)
        lone.close(); alone.close()
    assert np.array_equal(tr.read()[1], rec)               # detached, still readable
    tr.close()


# ---- 4. independence of what else is attached, of `every` and of the capacity ---------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders_every_or_capacity(pkg):
    n = (13, 10, 6)
    probe = _lattice(pkg, n, "noisy")
    levels = _levels(_field(pkg, probe, "hydrovs", "phi"), "above")[1:4]
    probe.close()
    records = {}
    for order in ("alone", "after the others"):
        lbm = _lattice(pkg, n, "noisy")
        others = []
        if order != "alone":
            others = [lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1), lbm.histogram_trace({"phi": (0.4, 0.6, 16)}, every=1, capacity=8),
                      lbm.morphology_trace("phi", levels, every=1, capacity=8), lbm.cluster_trace("rho", levels, side="below", connectivity=6, every=1, capacity=8)]
        tr = lbm.cluster_trace("phi", levels, every=2 if order == "alone" else 1, capacity=3 if order == "alone" else 16)
        lbm.LBM_timestep(6)
        assert all(r.count == 6 for r in others)
        records[order] = tr.read()
        lbm.close(); tr.close()
    steps, rec = records["alone"]
    assert steps[:, 0].tolist() == [7, 9, 11] and not np.array_equal(rec[0], rec[2])
    steps2, rec2 = records["after the others"]
    assert steps2[:, 0].tolist() == [6, 7, 8, 9, 10, 11]
    assert np.array_equal(rec2[1::2], rec)


# ---- 5. the lifecycle -----------------------------------------------------------------------------------------------------------
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
    tr = o.cluster_trace("rho", [0.999, 1.0, 1.001], every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="cluster trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    assert tr.count == 1 and tr.read()[0][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    tr.labels(1)                                                         # neither do the labels
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    steps, rec = tr.read()
    with pytest.raises(pkg.BflbmError, match="cluster trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="cluster trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, rec2 = tr.read()
    assert np.array_equal(rec, rec2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    w_steps, w_rec = tr.read(first=1, count=2)                            # a window of the record
    assert np.array_equal(w_rec, rec[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[0][0, 0] == 7
    # the owner goes first: the trace stays readable with the same integers, refuses a sample and labels, closes twice
    steps, rec = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, rec2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(rec, rec2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    with pytest.raises(pkg.BflbmError, match="bflbm_cluster_labels.*destroyed"):
        tr.labels()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm = _lattice(pkg, n, "noisy")
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_cluster_create.*replica of a batch.*use bflbm_batch_cluster_create"):
        batch.replicas[0].cluster_trace("rho", [1.0])
    lib = pkg._lib.load()
    for owner, call in ((lbm, "bflbm_cluster_create"), (batch, "bflbm_batch_cluster_create")):
        nrep = 3 if owner is batch else 1
        # (pattern, source, var, levels, side, connectivity, every, capacity), straight through the ABI: past the wrapper's own checks
        for pattern, source, var, levels, side, connectivity, every, capacity in (
                ("1..8 levels \\(got 0\\)", 0, 0, [], 0, 18, 1, 4),
                ("1..8 levels \\(got 9\\)", 0, 0, [0.5] * 9, 0, 26, 1, 4),
                ("level 1 is not finite \\(got nan\\)", 0, 0, [0.5, np.nan], 0, 26, 1, 4),
                ("level 0 is not finite \\(got inf\\)", 0, 0, [np.inf], 2, 18, 1, 4),
                ("side must be 0 \\(v >= level\\) or 1 \\(v < level\\) \\(got 2\\)", 0, 0, [0.5], 2, 18, 1, 4),
                ("source must be 0 \\(hydrovs\\) or 1 \\(hydrovsbar\\) \\(got 2\\)", 2, 0, [0.5], 0, 18, 1, 4),
                ("variable index 22 outside hydrovs \\(0..21\\)", 0, 22, [0.5], 0, 18, 1, 4),
                ("variable index 9 outside hydrovsbar \\(0..8\\)", 1, 9, [0.5], 0, 26, 1, 4),
                ("connectivity must be 6 or 26 \\(got 18\\)", 0, 0, [0.5], 0, 18, 0, 0),
                ("connectivity must be 6 or 26 \\(got 0\\)", 0, 0, [0.5], 0, 0, 1, 4),
                ("connectivity must be 6 or 26 \\(got -26\\)", 1, 0, [0.5], 1, -26, 1, 4),
                ("every must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 6, 0, 4),
                ("capacity must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 26, 1, 0),
                ("exceeds 1 TB", 0, 0, [0.5], 0, 26, 1, (1 << 37) // (cs.WORDS * nrep) + 1)):
            h = ctypes.c_void_p()
            lv = (ctypes.c_double * max(len(levels), 1))(*levels)
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                pkg._lib.check(getattr(lib, call)(owner._h, source, var, len(levels), lv, side, connectivity, every, capacity, ctypes.byref(h)))
            assert call in str(e.value) and not h.value, (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        # the limits themselves: 8 levels of the last component of either source
        for source, var in (("hydrovs", 21), ("hydrovsbar", 8)):
            full = owner.cluster_trace(var, np.linspace(-1.0, 1.0, 8), source=source, connectivity=6, capacity=1)
            full.sample()
            assert full.geometry()[0] == 8 and full.read()[1].shape == (1, nrep, 8, cs.WORDS)
            with pytest.raises(pkg.BflbmError, match="bflbm_cluster_labels: level index 8 outside 0..7"):
                full.labels(8)
            with pytest.raises(pkg.BflbmError, match="level index -1 outside"):
                full.labels(-1)
            full.close()
    for bad in (lambda: lbm.cluster_trace("no_such_variable", [1.0]), lambda: lbm.cluster_trace(["rho", "phi"], [1.0]),
                lambda: lbm.cluster_trace("rho", [1.0], side="left"), lambda: lbm.cluster_trace("rho", [1.0], source="noise"),
                lambda: lbm.cluster_trace("rho", [[1.0]]), lambda: lbm.cluster_trace("rho", [1.0], connectivity=18)):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_cluster_create inside an open step"):
        lbm.cluster_trace("rho", [1.0])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.cluster_trace("rho", [1.0], capacity=2)
    both = lbm.cluster_trace("rho", [1.0], side="below", capacity=2)       # an owner carries several: both sides
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset, tr.labels):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [6, 7]       # the split step samples in its finish
    assert both.count == 1 and tr.read()[1][1, 0, 0, 1] + both.read()[1][0, 0, 0, 1] == 512
    lbm.close(); batch.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_cluster_create.*nranks > 1"):
        slab.cluster_trace("rho", [1.0])
    slab.close()


# ---- 6. physics -----------------------------------------------------------------------------------------------------------------
def test_droplet_is_one_component_and_so_is_its_complement(pkg):
    """A 32^3 droplet after 5 zero-noise steps at the level midway between the extremes of its rho: one component under
    both connectivities, its label the mask's first site, ncomp == chi of a morphology trace; the complement is one
    component too."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=2.5), schedule="fused")
    lbm.LBM_init_droplet(0.3)
    lbm.LBM_timestep(5)
    rho = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(rho.max()) + float(rho.min()))
    mask = rho >= level
    assert 0 < mask.sum() < mask.size
    first = int(np.flatnonzero(mask.ravel())[0])
    mt = lbm.morphology_trace("rho", level, capacity=1)
    mt.sample()
    chi = int(mt.functionals()[0, 0, 0, 3])
    traces = [mt]
    for connectivity in cs.CONNECTIVITIES:
        tr = lbm.cluster_trace("rho", level, connectivity=connectivity, capacity=1)
        rec, _ = _check(pkg, tr, rho, [level], "above", connectivity)
        assert rec[0, :4].tolist() == [1, int(mask.sum()), int(mask.sum()), first] and rec[0, 0] == chi
        out = lbm.cluster_trace("rho", level, side="below", connectivity=connectivity, capacity=1)
        rec, _ = _check(pkg, out, rho, [level], "below", connectivity)
        assert rec[0, :4].tolist() == [1, int((~mask).sum()), int((~mask).sum()), 0]
        traces += [tr, out]
    print("droplet: V = %d, first site %d, chi = %d" % (mask.sum(), first, chi))
    lbm.close()
    for tr in traces:
        tr.close()


def test_spinodal_record_equals_the_twin_at_both_ends(pkg):
    """A 32^3 mixture at alpha0 = 2.5, kBT = 1e-5 sampled every 50 of 300 steps at the mean of phi: the first and the
    last sample equal the twin of the downloaded field.  ncomp(t) and smax / V are printed, not asserted: nobody has
    recorded them."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5, kBT=1e-5, seed=5), schedule="fused")
    lbm.LBM_init_mixture()
    level = float(_field(pkg, lbm, "hydrovs", "phi").mean())
    tr = lbm.cluster_trace("phi", level, every=50, capacity=7)
    tr.sample()
    assert np.array_equal(tr.read()[1][0, 0], pkg.analysis.cluster_record(_field(pkg, lbm, "hydrovs", "phi"), [level]))
    lbm.LBM_timestep(300)
    steps, rec = tr.read()
    assert steps[:, 0].tolist() == [0, 50, 100, 150, 200, 250, 300]
    assert np.array_equal(rec[-1, 0], pkg.analysis.cluster_record(_field(pkg, lbm, "hydrovs", "phi"), [level]))
    _assert_identities(rec, 32 ** 3)
    for k, step in enumerate(steps[:, 0]):
        print("spinodal step %4d: ncomp = %5d  V = %6d  smax / V = %.4f" % (step, rec[k, 0, 0, 0], rec[k, 0, 0, 1], rec[k, 0, 0, 2] / max(rec[k, 0, 0, 1], 1)))
    lbm.close(); tr.close()
