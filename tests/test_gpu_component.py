"""GPU: component traces (ComponentTrace, bflbm_component_*): per connected component of a thresholded field its size,
origin, extent, integer moments and area, recorded on the device as 64-bit integers.

The definition and the layout of a sample are in include/bflbm.h ("Component traces"); analysis.component_table restates
the rule in numpy and tests/test_component_abi.py holds it to an independent construction and to the closed forms.  Here
the device header and rows are compared with the twin of the field the same lattice hands out, integer for integer: lone
lattices of both sources, both sides, both connectivities and the three (min_size, rows) pairs, replicas of a batch,
planted sets, a box whose second moments pass 2^32.  Every case asserts first, from the twin or from the geometry, that
the condition it is there for really occurs.  Header word 5 (capped) is only ever asserted to be zero: no test provokes
the cap."""
import ctypes

import numpy as np
import pytest

import cluster_sets as cs
import component_sets as ks
from test_gpu_cluster import _planted
from test_gpu_morph import _batch_params, _field, _lattice

pytestmark = pytest.mark.gpu

BOXES = {(7, 3, 3): "one ragged brick that wraps onto itself",
         (32, 6, 5): "the x extent is the brick's: a brick's 32 x bits fill half a mask word",
         (70, 30, 6): "ragged bricks on every axis, two mask words along x: 70 = 2 x 32 + 6",
         (34, 31, 19): "ragged bricks on every axis, 80 bricks",
         (2, 2, 2): "the + and - neighbours coincide along every axis",
         (1, 3, 2): "a site is its own neighbour along x"}
STATES = ["stripe", "noisy", "random", "planted"]
FILLS = [0.05, 0.31, 0.9]                # sparse; near the 6-neighbour site-percolation threshold; one component holds nearly all
VARIABLES = {"hydrovs": "phi", "hydrovsbar": "rho"}


def _levels(x, side):
    """Three levels that are site values (equality is hit), at which the occupied fraction of the finite sites is about
    FILLS on the given side."""
    values = np.sort(x[np.isfinite(x)].ravel())
    qs = FILLS if side == "below" else [1.0 - q for q in FILLS]
    return [float(values[min(int(q * len(values)), len(values) - 1)]) for q in qs]


def _assert_identities(header, rows, n, nrows_max):
    """What holds for every record: header[..., 6], rows[..., R, 18] on the box n = (nx, ny, nz)."""
    sites = n[0] * n[1] * n[2]
    for h, t in zip(np.asarray(header).reshape(-1, 6).tolist(), np.asarray(rows).reshape(-1, nrows_max, 18).tolist()):
        ncomp, vol, nqual, vqual, nrows, capped = h
        assert capped == 0 and 0 <= nqual <= ncomp <= vol <= sites and nqual <= vqual <= vol and nrows == min(nqual, nrows_max)
        labels = [r[0] for r in t[:nrows]]
        assert labels == sorted(set(labels)) and all(0 <= v < sites for v in labels)
        assert all(r == [-1] + [0] * 17 for r in t[nrows:])
        for r in t[:nrows]:
            assert 1 <= r[1] <= vol and all(0 <= o < m and 1 <= e <= m for o, e, m in zip(r[2:5], r[5:8], n))
            assert max(r[5:8]) <= r[1] <= r[5] * r[6] * r[7] and 0 <= r[17] <= 6 * r[1]
            assert all(r[8 + a] <= r[1] * (r[5 + a] - 1) and r[8 + a] <= r[11 + a] for a in range(3))
        if nqual <= nrows_max:
            assert sum(r[1] for r in t) == vqual


def _check(pkg, tr, x, levels, side, connectivity, min_size, rows):
    """One sample of a lone trace against the twin of x; returns (header[nlevels, 6], rows[nlevels, rows, 18])."""
    tr.sample()
    steps, header, table = tr.read()
    want_h, want_t = pkg.analysis.component_table(x, levels, side, connectivity, min_size, rows)
    assert header.shape == (1, 1, len(levels), 6) and table.shape == (1, 1, len(levels), rows, 18) and header.dtype == table.dtype == np.int64
    assert np.array_equal(header[0, 0], want_h), (side, connectivity, min_size, rows, header[0, 0].tolist(), want_h.tolist())
    assert np.array_equal(table[0, 0], want_t), (side, connectivity, min_size, rows, np.argwhere(table[0, 0] != want_t)[:8].tolist())
    return header[0, 0], table[0, 0]


# ---- 1. a lone lattice against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,state", [(n, s) for n in BOXES for s in STATES])
def test_lone_header_and_rows_equal_the_twin(pkg, n, state):
    lbm = _lattice(pkg, n, state)
    steps_done = lbm.steps_done
    if n == (7, 3, 3):
        assert cs.bricks(n) == 1 and all(e < b for e, b in zip(n, cs.BRICK))
    if n in ((70, 30, 6), (34, 31, 19)):
        assert all(e % b for e, b in zip(n, cs.BRICK)) and cs.bricks(n) > 1
    traces = []
    overflowed = fitted = 0
    for source, name in VARIABLES.items():
        x = _field(pkg, lbm, source, name)
        for side in ("above", "below"):
            levels = _levels(x, side)
            for connectivity in cs.CONNECTIVITIES:
                for min_size, rows in ks.PAIRS:
                    tr = lbm.component_trace(name, levels, side=side, connectivity=connectivity, min_size=min_size, rows=rows, source=source, capacity=1)
                    traces.append(tr)
                    assert tr.geometry() == ks.geometry(3, connectivity, min_size, rows)
                    header, table = _check(pkg, tr, x, levels, side, connectivity, min_size, rows)
                    _assert_identities(header, table, n, rows)
                    assert tr.read()[0].tolist() == [[steps_done]] and tr.names == [name]
                    overflowed += int((header[:, 2] > rows).sum())
                    fitted += int(((header[:, 2] > 0) & (header[:, 2] <= rows)).sum())
                    assert np.array_equal(tr.sizes()[0, 0], table[..., 1]) and np.array_equal(tr.labels_of_rows()[0, 0], table[..., 0])
                    assert np.array_equal(tr.areas()[0, 0], table[..., 17])
                    assert np.array_equal(tr.spans()[0, 0], (table[..., 0:1] >= 0) & (table[..., 5:8] == np.array(n)))
                    if state == "random" and source == "hydrovs" and (min_size, rows) == (1, 256) and n in ((34, 31, 19), (70, 30, 6)):
                        frac = header[:, 1] / x.size
                        assert np.allclose(frac, FILLS, atol=0.01), frac
                        for l in ((1, 2) if connectivity == 26 else (2,)):      # above the threshold: a tabulated component across bricks and all three periodic planes
                            lab = pkg.analysis.cluster_labels(x, levels[l], side, connectivity)
                            big = int(table[l, np.argmax(table[l, :, 1]), 0])
                            assert len(cs.bricks_of(lab, big)) >= 2 and cs.wrapped_axes(lab, big, connectivity) == {0, 1, 2}
                        if connectivity == 26:                                  # at 0.05: small components that lie across a plane without spanning
                            sparse = table[0, :int(header[0, 4])]
                            assert ((sparse[:, 2:5] + sparse[:, 5:8] > np.array(n)) & (sparse[:, 5:8] < np.array(n))).any()
    if n in ((70, 30, 6), (34, 31, 19)) and state in ("noisy", "random"):
        assert overflowed and fitted                       # both more qualifying components than rows, and fewer
    if state == "planted":                                 # a NaN occupies nothing on either side
        assert np.isnan(_field(pkg, lbm, "hydrovs", "phi")).any()
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 2. planted sets ------------------------------------------------------------------------------------------------------------
def _sets(n):
    nx, ny, nz = n
    shape = (nz, ny, nx)
    slabs = np.zeros(shape, dtype=bool)
    slabs[[nz - 1, 0]] = True                              # across the periodic plane
    slabs[nz // 2] = True
    return {"snake": cs.snake(shape), "full": np.ones(shape, dtype=bool), "empty": np.zeros(shape, dtype=bool), "slabs": slabs,
            "cuboid": ks.corner_cuboid(shape, nx - 3, 3, 2)}


@pytest.mark.parametrize("n", [(34, 31, 19), (32, 6, 6)])
@pytest.mark.parametrize("which", ["snake", "full", "empty", "slabs", "cuboid"])
def test_planted_sets_equal_their_closed_forms_and_the_twin(pkg, n, which):
    nx, ny, nz = n
    mask = _sets(n)[which]
    sites = mask.size
    lbm = _planted(pkg, n, mask)
    x = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(x.max()) + float(x.min())) if which not in ("full", "empty") else (0.5 if which == "full" else 2.0)
    assert np.array_equal(x >= level, mask)                # the set on the device is the set that was planted
    unused = [-1] + [0] * 17
    traces = []
    for connectivity in cs.CONNECTIVITIES:
        tr = lbm.component_trace("rho", level, connectivity=connectivity, rows=4, capacity=1)
        traces.append(tr)
        header, table = _check(pkg, tr, x, [level], "above", connectivity, 1, 4)
        h, t = header[0].tolist(), table[0].tolist()
        v = int(mask.sum())
        if which == "snake":                               # one component through every brick: every brick flushes into one row
            lab = cs.flood(mask, connectivity)
            assert len(cs.bricks_of(lab, 0)) == cs.bricks(n) > 1
            assert h == [1, v, 1, v, 1, 0] and t[0][:2] == [0, v] and t[1:] == [unused] * 3 and t[0] == ks.table(mask, connectivity, 1, 4)[1][0]
        if which == "full":
            assert h == [1, sites, 1, sites, 1, 0] and t[0][:8] == [0, sites, 0, 0, 0, nx, ny, nz] and t[0][17] == 0
            assert t[0][8:11] == [sites * (e - 1) // 2 for e in n] and t[0][14] == sites * (nx - 1) * (ny - 1) // 4
            assert tr.spans()[0, 0, 0, 0].tolist() == [True] * 3 and np.isnan(tr.centroids()[0, 0, 0, 0]).all()
        if which == "empty":
            assert h == [0] * 6 and t == [unused] * 4
        if which == "slabs":
            plane = nx * ny
            assert h == [2, 3 * plane, 2, 3 * plane, 2, 0]
            assert t[0][:8] == [0, 2 * plane, 0, 0, nz - 1, nx, ny, 2] and t[1][:8] == [(nz // 2) * plane, plane, 0, 0, nz // 2, nx, ny, 1]
            assert t[0][17] == t[1][17] == 2 * plane and t[0][10] == plane and t[1][10] == 0
            assert tr.spans()[0, 0, 0, :2].tolist() == [[True, True, False]] * 2
        if which == "cuboid":
            assert h == [1, v, 1, v, 1, 0] and t[0] == ks.cuboid_row(mask.shape, nx - 3, 3, 2) and t[0][17] == 2 * ((nx - 3) * 3 + 3 * 2 + 2 * (nx - 3))
            assert tr.spans()[0, 0, 0, 0].tolist() == [False] * 3
            centre = tr.centroids()[0, 0, 0, 0]
            assert np.allclose(centre, np.mod([nx - 1 + (nx - 4) / 2, ny - 1 + 1.0, nz - 1 + 0.5], n))
    lbm.close()
    for tr in traces:
        tr.close()


# ---- 3. sums beyond 32 bits -------------------------------------------------------------------------------------------------------
def test_full_box_second_moment_passes_two_to_the_32(pkg):
    """The full (512, 16, 16) box: sum x^2 = 256 x 511 x 512 x 1023 / 6 = 11 419 713 536 > 2^32, the smallest shape at which
    a 32-bit global sum breaks; the closed forms of every word."""
    n = (512, 16, 16)
    nx, ny, nz = n
    sites = nx * ny * nz
    lbm = _planted(pkg, n, np.ones((nz, ny, nx), dtype=bool))
    tr = lbm.component_trace("rho", 0.5, connectivity=6, rows=2, capacity=1)
    tr.sample()
    _, header, table = tr.read()
    row = table[0, 0, 0, 0].tolist()
    want = ([0, sites, 0, 0, 0, nx, ny, nz] + [sites * (e - 1) // 2 for e in n] + [sites * (e - 1) * (2 * e - 1) // 6 for e in n] +
            [sites * (nx - 1) * (ny - 1) // 4, sites * (nx - 1) * (nz - 1) // 4, sites * (ny - 1) * (nz - 1) // 4, 0])
    assert want[11] == 11419713536 > 2 ** 32
    assert header[0, 0, 0].tolist() == [1, sites, 1, sites, 1, 0] and row == want and table[0, 0, 0, 1].tolist() == [-1] + [0] * 17
    lbm.close(); tr.close()


# ---- 4. against the cluster trace and the morphology trace ------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", cs.CONNECTIVITIES)
def test_rows_agree_with_the_cluster_and_morphology_traces(pkg, connectivity):
    n = (34, 31, 19)
    lbm = _lattice(pkg, n, "random")
    x = _field(pkg, lbm, "hydrovs", "phi")
    levels = _levels(x, "below")[1:]                         # fills 0.31 and 0.9: few enough components for 256 rows at 26
    ct = lbm.cluster_trace("phi", levels, side="below", connectivity=connectivity, capacity=1)
    mt = lbm.morphology_trace("phi", levels, side="below", capacity=1)
    tr = lbm.component_trace("phi", levels, side="below", connectivity=connectivity, min_size=1, rows=256, capacity=1)
    for r in (ct, mt, tr):
        r.sample()
    rec = ct.read()[1][0, 0]
    area = pkg.analysis.minkowski_functionals(mt.read()[1])[0, 0, :, 1]
    _, header, table = tr.read()
    header, table = header[0, 0], table[0, 0]
    assert np.array_equal(header[:, :2], rec[:, :2]) and (header[:, 5] == 0).all()
    fits = header[:, 2] <= 256
    assert fits.any()                                      # at least one level whose components all have a row
    for l in np.flatnonzero(fits):
        assert table[l, :, 17].sum() == area[l] and table[l, :, 1].sum() == header[l, 1]
        big = np.lexsort((table[l, :, 0], -table[l, :, 1]))[0]                 # the largest size, among equals the smallest label
        assert table[l, big, 1] == rec[l, 2] and table[l, big, 0] == rec[l, 3]
    lbm.close()
    for r in (ct, mt, tr):
        r.close()


# ---- 5. a batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,name,side,connectivity,pair", [("hydrovs", "phi", "above", 26, (3, 16)), ("hydrovsbar", "rho", "below", 6, (1, 4))])
def test_batch_replicas_equal_the_twin_and_the_lattice_run_alone(pkg, source, name, side, connectivity, pair):
    n = (34, 31, 19)
    min_size, rows = pair
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    batch.LBM_timestep(3)
    levels = _levels(_field(pkg, batch.replicas[0], source, name), side)      # one set of levels for all replicas
    make = dict(side=side, connectivity=connectivity, min_size=min_size, rows=rows, source=source, every=2, capacity=4)
    tr = batch.component_trace(name, levels, **make)
    assert tr.geometry() == ks.geometry(3, connectivity, min_size, rows)
    tr.sample()
    steps, header, table = tr.read()
    assert steps.tolist() == [[3, 1003, 3]] and header.shape == (1, 3, 3, 6) and table.shape == (1, 3, 3, rows, 18)
    _assert_identities(header, table, n, rows)
    for r, v in enumerate(batch.replicas):
        want_h, want_t = pkg.analysis.component_table(_field(pkg, v, source, name), levels, side, connectivity, min_size, rows)
        assert np.array_equal(header[0, r], want_h) and np.array_equal(table[0, r], want_t), (source, r)
    assert not np.array_equal(table[0, 0], table[0, 1]) and not np.array_equal(table[0, 0], table[0, 2])
    batch.LBM_timestep(4)                                  # samples after the batch steps 2 and 4
    steps, header, table = tr.read()
    assert steps[:, 0].tolist() == [3, 5, 7]
    batch.close()
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        if r == 1:
            lone.set_steps_done(1000)
        lone.LBM_timestep(3)
        alone = lone.component_trace(name, levels, **make)
        alone.sample()
        lone.LBM_timestep(4)
        a_steps, a_header, a_table = alone.read()
        assert np.array_equal(a_steps[:, 0], steps[:, r]) and np.array_equal(a_header[:, 0], header[:, r]) and np.array_equal(a_table[:, 0], table[:, r]), (source, r)
        lone.close(); alone.close()
    assert np.array_equal(tr.read()[2], table)             # detached, still readable
    tr.close()


# ---- 6. independence of what else is attached, of `every` and of the capacity ---------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders_every_or_capacity(pkg):
    n = (13, 10, 6)
    probe = _lattice(pkg, n, "noisy")
    levels = _levels(_field(pkg, probe, "hydrovs", "phi"), "above")
    probe.close()
    records = {}
    for order in ("alone", "after the others"):
        lbm = _lattice(pkg, n, "noisy")
        others = []
        if order != "alone":
            others = [lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1), lbm.morphology_trace("phi", levels, every=1, capacity=8),
                      lbm.cluster_trace("phi", levels, every=1, capacity=8),
                      lbm.component_trace("rho", levels, side="below", connectivity=6, min_size=2, rows=3, every=1, capacity=8)]
        tr = lbm.component_trace("phi", levels, rows=16, every=2 if order == "alone" else 1, capacity=3 if order == "alone" else 16)
        lbm.LBM_timestep(6)
        assert all(r.count == 6 for r in others)
        records[order] = tr.read()
        lbm.close(); tr.close()
        for r in others:
            r.close()
    steps, header, table = records["alone"]
    assert steps[:, 0].tolist() == [7, 9, 11] and not np.array_equal(table[0], table[2])
    steps2, header2, table2 = records["after the others"]
    assert steps2[:, 0].tolist() == [6, 7, 8, 9, 10, 11]
    assert np.array_equal(header2[1::2], header) and np.array_equal(table2[1::2], table)


# ---- 7. the lifecycle -----------------------------------------------------------------------------------------------------------
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
    tr = o.component_trace("rho", [0.999, 1.0, 1.001], rows=8, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="component trace full"):
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
    steps, header, table = tr.read()
    with pytest.raises(pkg.BflbmError, match="component trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="component trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, header2, table2 = tr.read()
    assert np.array_equal(table, table2) and np.array_equal(header, header2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    w_steps, w_header, w_table = tr.read(first=1, count=2)                # a window of the record
    assert np.array_equal(w_table, table[1:]) and np.array_equal(w_header, header[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[2].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[0][0, 0] == 7
    # the owner goes first: the trace stays readable with the same integers, refuses a sample, closes twice
    steps, header, table = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, header2, table2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(header, header2) and np.array_equal(table, table2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm = _lattice(pkg, n, "noisy")
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_component_create.*replica of a batch.*use bflbm_batch_component_create"):
        batch.replicas[0].component_trace("rho", [1.0])
    lib = pkg._lib.load()
    for owner, call in ((lbm, "bflbm_component_create"), (batch, "bflbm_batch_component_create")):
        nrep = 3 if owner is batch else 1
        # (pattern, source, var, levels, side, connectivity, min_size, rows, every, capacity), straight through the ABI
        for pattern, source, var, levels, side, connectivity, min_size, rows, every, capacity in (
                ("1..8 levels \\(got 0\\)", 0, 0, [], 0, 18, 0, 0, 1, 4),
                ("1..8 levels \\(got 9\\)", 0, 0, [0.5] * 9, 0, 26, 1, 4, 1, 4),
                ("level 1 is not finite \\(got nan\\)", 0, 0, [0.5, np.nan], 0, 26, 1, 4, 1, 4),
                ("side must be 0 \\(v >= level\\) or 1 \\(v < level\\) \\(got 2\\)", 0, 0, [0.5], 2, 18, 0, 0, 1, 4),
                ("source must be 0 \\(hydrovs\\) or 1 \\(hydrovsbar\\) \\(got 2\\)", 2, 0, [0.5], 0, 18, 0, 0, 1, 4),
                ("variable index 22 outside hydrovs \\(0..21\\)", 0, 22, [0.5], 0, 18, 0, 0, 1, 4),
                ("variable index 9 outside hydrovsbar \\(0..8\\)", 1, 9, [0.5], 0, 26, 1, 4, 1, 4),
                ("connectivity must be 6 or 26 \\(got 18\\)", 0, 0, [0.5], 0, 18, 0, 0, 0, 0),
                ("min_size must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 26, 0, 0, 0, 0),
                ("min_size must be >= 1 \\(got -3\\)", 0, 0, [0.5], 0, 6, -3, 4, 1, 4),
                ("rows must be in 1..256 \\(got 0\\)", 0, 0, [0.5], 0, 26, 1, 0, 0, 0),
                ("rows must be in 1..256 \\(got 257\\)", 0, 0, [0.5], 0, 26, 1, 257, 1, 4),
                ("every must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 6, 1, 4, 0, 4),
                ("capacity must be >= 1 \\(got 0\\)", 0, 0, [0.5], 0, 26, 1, 4, 1, 0),
                ("exceeds 1 TB", 0, 0, [0.5], 0, 26, 1, 4, 1, (1 << 37) // ((6 + 4 * 18) * nrep) + 1)):
            h = ctypes.c_void_p()
            lv = (ctypes.c_double * max(len(levels), 1))(*levels)
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                pkg._lib.check(getattr(lib, call)(owner._h, source, var, len(levels), lv, side, connectivity, min_size, rows, every, capacity, ctypes.byref(h)))
            assert call in str(e.value) and not h.value, (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        # the limits themselves: 8 levels of the last component of either source, 256 rows, a min_size no component reaches
        for source, var in (("hydrovs", 21), ("hydrovsbar", 8)):
            full = owner.component_trace(var, np.linspace(-1.0, 1.0, 8), source=source, connectivity=6, min_size=2 ** 40, rows=256, capacity=1)
            full.sample()
            steps, header, table = full.read()
            assert full.geometry() == ks.geometry(8, 6, 2 ** 40, 256) and header.shape == (1, nrep, 8, 6) and table.shape == (1, nrep, 8, 256, 18)
            assert (header[..., 2:5] == 0).all() and (table[..., 0] == -1).all() and (header[..., 0] <= header[..., 1]).all()
            full.close()
    for bad in (lambda: lbm.component_trace("no_such_variable", [1.0]), lambda: lbm.component_trace(["rho", "phi"], [1.0]),
                lambda: lbm.component_trace("rho", [1.0], side="left"), lambda: lbm.component_trace("rho", [1.0], source="noise"),
                lambda: lbm.component_trace("rho", [[1.0]]), lambda: lbm.component_trace("rho", [1.0], connectivity=18)):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_component_create inside an open step"):
        lbm.component_trace("rho", [1.0])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.component_trace("rho", [1.0], capacity=2)
    both = lbm.component_trace("rho", [1.0], side="below", capacity=2)     # an owner carries several: both sides
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [6, 7]       # the split step samples in its finish
    assert both.count == 1 and tr.read()[1][1, 0, 0, 1] + both.read()[1][0, 0, 0, 1] == 512
    lbm.close(); batch.close()
    tr.close(); both.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_component_create.*nranks > 1"):
        slab.component_trace("rho", [1.0])
    slab.close()


# ---- 8. physics -----------------------------------------------------------------------------------------------------------------
def test_droplet_is_one_row_and_its_complement_spans(pkg):
    """A 32^3 droplet after 5 zero-noise steps at the level midway between the extremes of its rho: one row, its centroid
    the numpy centroid of the mask, no axis spanned; the complement spans every axis.  The radius of gyration against the
    sphere's 3 R^2 / 5 with R from the row's size is printed, not asserted: a voxelised ball is not a sphere."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=2.5), schedule="fused")
    lbm.LBM_init_droplet(0.3)
    lbm.LBM_timestep(5)
    rho = _field(pkg, lbm, "hydrovs", "rho")
    level = 0.5 * (float(rho.max()) + float(rho.min()))
    mask = rho >= level
    z, y, x = np.nonzero(mask)
    assert 0 < mask.sum() < mask.size and x.min() > 0 and x.max() < 31 and y.min() > 0 and z.min() > 0     # clear of the periodic planes
    traces = []
    for connectivity in cs.CONNECTIVITIES:
        tr = lbm.component_trace("rho", level, connectivity=connectivity, rows=4, capacity=1)
        header, table = _check(pkg, tr, rho, [level], "above", connectivity, 1, 4)
        assert header[0].tolist() == [1, int(mask.sum()), 1, int(mask.sum()), 1, 0]
        assert np.allclose(tr.centroids()[0, 0, 0, 0], [x.mean(), y.mean(), z.mean()], rtol=0, atol=1e-12)
        assert not tr.spans()[0, 0, 0].any() and np.isnan(tr.centroids()[0, 0, 0, 1:]).all()
        g = tr.gyration()[0, 0, 0, 0]
        radius = (3.0 * mask.sum() / (4.0 * np.pi)) ** (1.0 / 3.0)
        print("droplet (%d): V = %d, trace(gyration) = %.4f, 3 R^2 / 5 = %.4f, area = %d" % (connectivity, mask.sum(), np.trace(g), 0.6 * radius ** 2, table[0, 0, 17]))
        out = lbm.component_trace("rho", level, side="below", connectivity=connectivity, rows=4, capacity=1)
        header, table = _check(pkg, out, rho, [level], "below", connectivity, 1, 4)
        assert header[0, :5].tolist() == [1, int((~mask).sum()), 1, int((~mask).sum()), 1] and out.spans()[0, 0, 0, 0].all()
        traces += [tr, out]
    lbm.close()
    for tr in traces:
        tr.close()


def test_spinodal_rows_equal_the_twin_at_both_ends(pkg):
    """A 32^3 mixture at alpha0 = 2.5, kBT = 1e-5 sampled every 50 of 300 steps at the mean of phi: the first and the last
    sample equal the twin of the downloaded field.  nqual(t) and the spanning flags are printed, not asserted: nobody has
    recorded them."""
    n = (32, 32, 32)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5, kBT=1e-5, seed=5), schedule="fused")
    lbm.LBM_init_mixture()
    level = float(_field(pkg, lbm, "hydrovs", "phi").mean())
    tr = lbm.component_trace("phi", level, min_size=3, rows=16, every=50, capacity=7)
    tr.sample()
    want = pkg.analysis.component_table(_field(pkg, lbm, "hydrovs", "phi"), [level], "above", 26, 3, 16)
    assert np.array_equal(tr.read()[1][0, 0], want[0]) and np.array_equal(tr.read()[2][0, 0], want[1])
    lbm.LBM_timestep(300)
    steps, header, table = tr.read()
    assert steps[:, 0].tolist() == [0, 50, 100, 150, 200, 250, 300]
    want = pkg.analysis.component_table(_field(pkg, lbm, "hydrovs", "phi"), [level], "above", 26, 3, 16)
    assert np.array_equal(header[-1, 0], want[0]) and np.array_equal(table[-1, 0], want[1])
    _assert_identities(header, table, n, 16)
    spans = tr.spans()
    for k, step in enumerate(steps[:, 0]):
        print("spinodal step %4d: ncomp = %5d  nqual = %5d  rows spanning x, y, z: %s" % (step, header[k, 0, 0, 0], header[k, 0, 0, 2], spans[k, 0, 0].sum(axis=0).tolist()))
    lbm.close(); tr.close()
