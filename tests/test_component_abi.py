"""Component traces, CPU side: analysis.component_table against the independent construction of tests/component_sets.py
(Python integers over flood-fill labels), the record's identities, the closed forms, the invariance under translation,
analysis.track_components, the C-ABI surface (declared, exported, bound with the header's argument lists), the
null-pointer refusals (which must fail before any device is touched), the host part of csrc/bflbm_components.h through a
stand-alone program built with the address and undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc
cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels, mangled   # noqa: F401  (device_asm: the listing fixture)

import cluster_sets as cs
import component_sets as ks
from test_cluster_abi import BOXES, FILLS
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

COMPONENT_SYMBOLS = ["bflbm_component_create", "bflbm_batch_component_create", "bflbm_component_destroy", "bflbm_component_sample",
                     "bflbm_component_reset", "bflbm_component_count", "bflbm_component_geometry", "bflbm_component_read"]


def _table(pkg, occ, connectivity, min_size=1, rows=256):
    """The twin's header and rows of a boolean set as lists: the field is the set itself, the level one half."""
    h, t = pkg.analysis.component_table(np.asarray(occ, dtype=np.float64), [0.5], "above", connectivity, min_size, rows)
    return h[0].tolist(), t[0].tolist()


# ---- the numpy twin against the independent construction ------------------------------------------------------------------
def test_component_table_against_the_independent_construction(pkg):
    an = pkg.analysis
    overflowing = fitting = 0
    for n in BOXES:
        nx, ny, nz = n
        rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
        for fill in FILLS:
            v = rng.random((nz, ny, nx))
            for connectivity in cs.CONNECTIVITIES:
                for side, level, occ in (("above", 1.0 - fill, v >= 1.0 - fill), ("below", fill, v < fill)):
                    for min_size, rows in ks.PAIRS:
                        want_h, want_t, single_arc = ks.table(occ, connectivity, min_size, rows)
                        assert single_arc, (n, fill, side, connectivity)       # every projection is one arc, or the axis
                        header, table = an.component_table(v, [level, 2.0 if side == "above" else -1.0], side, connectivity, min_size, rows)
                        assert header.dtype == table.dtype == np.int64 and header.shape == (2, 6) and table.shape == (2, rows, 18)
                        assert header[0].tolist() == want_h, (n, fill, side, connectivity, min_size, rows)
                        assert table[0].tolist() == want_t, (n, fill, side, connectivity, min_size, rows)
                        assert header[1].tolist() == [0] * 6 and table[1].tolist() == [[-1] + [0] * 17] * rows      # nothing occupied
                        overflowing += want_h[2] > rows
                        fitting += 0 < want_h[2] <= rows
                        # the identities of a record
                        rec = an.cluster_record(v, [level], side, connectivity)[0]
                        assert want_h[0] == rec[0] and want_h[1] == rec[1] == occ.sum() and want_h[4] == min(want_h[2], rows) and want_h[5] == 0
                        if want_h[2] <= rows:
                            assert sum(r[1] for r in want_t) == want_h[3]
                            if min_size == 1:
                                s = an.minkowski_functionals(an.minkowski_counts(v, [level], side))[0, 1]
                                assert sum(r[17] for r in want_t) == s
                                assert want_h[2] == want_h[0] and want_h[3] == want_h[1]
                        labels = [r[0] for r in want_t[:want_h[4]]]
                        assert labels == sorted(labels) and all(r[1] >= min_size for r in want_t[:want_h[4]])
    assert overflowing > 20 and fitting > 200                 # the inputs hold both


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def test_closed_forms(pkg):
    shape = (9, 8, 10)                                     # [nz, ny, nx]
    nz, ny, nx = shape
    sites = nz * ny * nx
    unused = [-1] + [0] * 17
    for c in cs.CONNECTIVITIES:
        # a cuboid planted across the periodic corner
        for a, b, d in ((3, 2, 4), (9, 7, 8), (2, 2, 2)):
            occ = ks.corner_cuboid(shape, a, b, d)
            h, t = _table(pkg, occ, c, 1, 4)
            assert h == [1, a * b * d, 1, a * b * d, 1, 0]
            assert t[0] == ks.cuboid_row(shape, a, b, d) and t[1:] == [unused] * 3
            assert t[0][17] == 2 * (a * b + b * d + d * a) and t[0][8] * 2 == a * b * d * (a - 1)
            assert ks.table(occ, c, 1, 4)[:2] == (h, t)
        # a slab across the periodic z plane spans x and y, not z
        slab = np.zeros(shape, dtype=bool)
        slab[[8, 0, 1]] = True
        h, t = _table(pkg, slab, c, 1, 2)
        assert h == [1, 240, 1, 240, 1, 0] and t[0][:8] == [0, 240, 0, 0, 8, nx, ny, 3] and t[0][17] == 2 * nx * ny
        assert t[0][10] == 80 * (0 + 1 + 2) and t[0][13] == 80 * (0 + 1 + 4)
        # the full box spans every axis and has no faces
        h, t = _table(pkg, np.ones(shape), c, 1, 1)
        assert h == [1, sites, 1, sites, 1, 0] and t[0][:8] == [0, sites, 0, 0, 0, nx, ny, nz] and t[0][17] == 0
        assert t[0][8] == sites * (nx - 1) // 2 and t[0][11] == sites * (nx - 1) * (2 * nx - 1) // 6
        # nothing
        assert _table(pkg, np.zeros(shape), c, 1, 3) == ([0] * 6, [unused] * 3)
        # a path that covers every x without a link across the x plane: it spans x and does not wrap
        path = np.zeros(shape, dtype=bool)
        path[4, 2, 0:6] = True
        path[4, 2:6, 5] = True
        path[4, 5, 5:10] = True
        h, t = _table(pkg, path, c, 1, 2)
        assert h[:5] == [1, 13, 1, 13, 1] and t[0][2:8] == [0, 2, 4, nx, 4, 1]
        assert cs.wrapped_axes(cs.flood(path, c), t[0][0], c) == set()
        path[4, 2, 0] = False                              # one x less: an arc again, from x = 1
        assert _table(pkg, path, c, 1, 2)[1][0][2:8] == [1, 2, 4, nx - 1, 4, 1]
        # min_size and rows: four cubes of 8, 1, 27 and 1 sites
        cubes = np.zeros(shape, dtype=bool)
        cubes[0:2, 0:2, 0:2] = cubes[4, 4, 4] = cubes[5:8, 0:3, 5:8] = cubes[8, 6, 0] = True
        h, t = _table(pkg, cubes, c, 2, 1)
        assert h == [4, 37, 2, 35, 1, 0] and t[0][:2] == [0, 8]
        h, t = _table(pkg, cubes, c, 9, 3)
        assert h == [4, 37, 1, 27, 1, 0] and t[0][:8] == [(5 * ny + 0) * nx + 5, 27, 5, 0, 5, 3, 3, 3] and t[1:] == [unused] * 2
    # the smallest boxes: the + and - neighbours coincide, or a site is its own neighbour
    for shape2, sites2 in (((2, 2, 2), 8), ((2, 3, 1), 6)):    # (nx, ny, nz) = (2, 2, 2) and (1, 3, 2)
        for c in cs.CONNECTIVITIES:
            h, t = _table(pkg, np.ones(shape2), c, 1, 2)
            assert h == [1, sites2, 1, sites2, 1, 0] and t[0][17] == 0 and t[0][5:8] == list(shape2[::-1])
            one = np.zeros(shape2, dtype=bool)
            one[0, 0, 0] = True
            h, t = _table(pkg, one, c, 1, 2)
            spanned = sum(e == 1 for e in shape2)          # along an axis of extent 1 the neighbour is the site itself
            assert t[0][:8] == [0, 1, 0, 0, 0, 1, 1, 1] and t[0][17] == 6 - 2 * spanned and t[0][8:17] == [0] * 9
            assert ks.table(one, c, 1, 2)[1] == t


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((3, 4, 5))
    for bad in (lambda: an.component_table(f, [0.0], min_size=0), lambda: an.component_table(f, [0.0], rows=0),
                lambda: an.component_table(f, [0.0], rows=257), lambda: an.component_table(f, [0.0], min_size=1.5),
                lambda: an.component_table(f, [0.0], "above", 18), lambda: an.component_table(f, []), lambda: an.component_table(f[0], [0.0]),
                lambda: an.track_components(np.zeros((2, 3)), np.zeros((2, 3)), (4, 4, 4), 1.0),
                lambda: an.track_components(np.zeros((2, 3, 3)), np.zeros((2, 3)), (4, 4, 4), 0.0)):
        with pytest.raises(ValueError):
            bad()
    h, t = an.component_table(f, 0.0)
    assert h.shape == (1, 6) and t.shape == (1, 256, 18)


# ---- translation --------------------------------------------------------------------------------------------------------------
def test_translation_leaves_the_shape_and_moves_the_centroid(pkg):
    an = pkg.analysis
    shape = (9, 9, 11)
    nz, ny, nx = shape
    z, y, x = np.indices(shape)
    blob = ((x - 4) ** 2 + 2 * (y - 3) ** 2 + (z - 4) ** 2 <= 9) | ((x == 6) & (y == 3) & (z < 5))     # no symmetry to hide behind
    h, t = _table(pkg, blob, 6)
    assert h[:5] == [1, int(blob.sum()), 1, int(blob.sum()), 1] and all(e < m for e, m in zip(t[0][5:8], (nx, ny, nz)))
    want = (t[0][1], t[0][5:8], t[0][17], ks.central(t[0]))
    centre = an.component_centroids(np.array(t[0]), (nx, ny, nz))
    crossings = set()
    for sz in range(nz):
        for sy in range(0, ny, 2):
            for sx in range(nx):
                moved = np.roll(blob, (sz, sy, sx), axis=(0, 1, 2))
                row = _table(pkg, moved, 6)[1][0]
                assert (row[1], row[5:8], row[17], ks.central(row)) == want, (sx, sy, sz)
                got = an.component_centroids(np.array(row), (nx, ny, nz))
                assert np.allclose(np.mod(got - centre - (sx, sy, sz) + 1.0, (nx, ny, nz)), 1.0, atol=1e-9), (sx, sy, sz)
                crossings.add(tuple(o + e > m for o, e, m in zip(row[2:5], row[5:8], (nx, ny, nz))))
    assert (True, True, True) in crossings and (False, False, False) in crossings      # the set lay across every plane, and across none
    g = an.component_gyration(np.array(t[0]))
    s = t[0][1]
    c = ks.central(t[0])
    assert g.shape == (3, 3) and np.allclose(np.diag(g), np.array(c[:3]) / s ** 2) and np.allclose([g[0, 1], g[0, 2], g[1, 2]], np.array(c[3:]) / s ** 2)
    assert np.array_equal(g, g.T)
    # unused rows and spanned axes
    full = np.array(_table(pkg, np.ones(shape), 6, 1, 2)[1])
    assert np.isnan(an.component_centroids(full, (nx, ny, nz))).all() and np.isnan(an.component_gyration(full)[1]).all()
    slab = np.zeros(shape, dtype=bool)
    slab[[nz - 1, 0]] = True
    cen = an.component_centroids(np.array(_table(pkg, slab, 6, 1, 1)[1][0]), (nx, ny, nz))
    assert np.isnan(cen[:2]).all() and cen[2] == nz - 0.5


# ---- tracking -------------------------------------------------------------------------------------------------------------------
def test_track_components_follows_two_points_across_the_origin(pkg):
    """Two planted points move at constant velocity; one crosses the box origin, so that the row order swaps: the
    trajectories are straight lines.  Then a birth and a loss."""
    an = pkg.analysis
    n = (12, 10, 8)
    steps = 8
    start = np.array([[2.0, 5.0, 4.0], [9.0, 4.0, 1.0]])
    velocity = np.array([[1.0, 0.5, 0.0], [-0.5, 0.0, -0.5]])
    cents = np.full((steps, 3, 3), np.nan)
    sizes = np.zeros((steps, 3), dtype=np.int64)
    orders = []
    for t in range(steps):
        pos = np.mod(start + t * velocity, n)
        label = (np.floor(pos[:, 2]) * n[1] + np.floor(pos[:, 1])) * n[0] + np.floor(pos[:, 0])
        order = np.argsort(label)                          # rows ascend with the label, as in a record
        orders.append(order.tolist())
        cents[t, :2], sizes[t, :2] = pos[order], 1
    assert [0, 1] in orders and [1, 0] in orders and orders[0] != orders[-1]        # the rows swap
    assert (start[1, 2] + (steps - 1) * velocity[1, 2]) < 0                            # a periodic plane is crossed
    tracks = an.track_components(cents, sizes, n, max_jump=2.0)
    assert tracks.shape == (2, steps, 3)
    first = orders[0]
    for k in range(2):
        assert np.allclose(tracks[k], start[first[k]] + np.arange(steps)[:, None] * velocity[first[k]])
    d = tracks - tracks[:, :1]
    assert np.allclose((d ** 2).sum(axis=-1)[:, -1], ((steps - 1) * velocity[first]) ** 2 @ np.ones(3))     # what analysis.msd is fed
    # a birth at sample 3 in row 2, the loss of the first track after sample 5
    cents[3:, 2], sizes[3:, 2] = [6.0, 8.0, 6.0], 5
    lost = first.index(0)
    for t in range(6, steps):
        row = orders[t].index(0)
        cents[t, row], sizes[t, row] = np.nan, 0
    tracks = an.track_components(cents, sizes, n, max_jump=2.0)
    assert tracks.shape == (3, steps, 3)
    assert np.isnan(tracks[2, :3]).all() and np.allclose(tracks[2, 3:], [6.0, 8.0, 6.0])
    assert np.isfinite(tracks[lost, :6]).all() and np.isnan(tracks[lost, 6:]).all() and np.isfinite(tracks[1 - lost]).all()
    # too far to be the same component: a loss and a birth
    far = an.track_components(np.array([[[1.0, 1.0, 1.0]], [[5.0, 1.0, 1.0]]]), np.ones((2, 1)), n, max_jump=2.0)
    assert far.shape == (2, 2, 3) and np.isnan(far[0, 1]).all() and np.isnan(far[1, 0]).all()
    # a tie goes to the smaller row
    tie = an.track_components(np.array([[[4.0, 1.0, 1.0], [np.nan] * 3], [[3.0, 1.0, 1.0], [5.0, 1.0, 1.0]]]), np.array([[1, 0], [1, 1]]), n, 2.0)
    assert tie.shape == (2, 2, 3) and tie[0, 1].tolist() == [3.0, 1.0, 1.0] and np.isnan(tie[1, 0]).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_component_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in COMPONENT_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_component_create"] == sig["bflbm_batch_component_create"]
    # (owner, source, var, nlevels, levels, side, connectivity, min_size, rows, every, capacity, out)
    create = sig["bflbm_component_create"][1]
    assert len(create) == 12 and create[7] is ctypes.c_longlong and create[8] is ctypes.c_int and create[10] is ctypes.c_longlong
    assert sig["bflbm_component_read"][1][3] == ctypes.POINTER(ctypes.c_longlong)        # integers, not doubles
    assert len(sig["bflbm_component_geometry"][1]) == 8 and sig["bflbm_component_geometry"][1][3] == ctypes.POINTER(ctypes.c_longlong)
    assert header.count("Component traces:") == 1 and header.count("Cluster traces:") == 1
    assert "bflbm_ring_component_create" not in sig and not hasattr(lib, "bflbm_ring_component_create")  # a ring is out of scope
    assert hasattr(pkg, "ComponentTrace") and "ComponentTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "component_trace")
    assert not hasattr(pkg.RingLBM, "component_trace")
    for fn in ("component_table", "component_centroids", "component_gyration", "track_components"):
        assert hasattr(pkg.analysis, fn)
    for method in ("read", "sizes", "labels_of_rows", "spans", "areas", "centroids", "gyration", "geometry", "names"):
        assert hasattr(pkg.ComponentTrace, method)
    # the header, the numpy twin, the tests' helper and the kernels' header state the same constants
    an = pkg.analysis
    assert (an.COMPONENT_HEADER, an.COMPONENT_ROW, an.COMPONENT_MAX_ROWS) == (ks.HEADER, ks.ROW, ks.MAX_ROWS) == (6, 18, 256)
    block = re.sub(r"\s*\n \*\s+", " ", header[header.index("Component traces:"):header.index("typedef struct bflbm_component")])
    for words in ("rows in 1..256", "[6 + rows x 18]", "the launches per level (%d)" % ks.LAUNCHES, "%d launches: k_cluster_local" % ks.LAUNCHES,
                  "a single arc, or all of it", "necessary for wrapping", "not sufficient", "S = -6 N3 + 2 N2", "2 P = 12 N3 - 2 N2",
                  "an extent above 65536 is refused", "2^31 2^32 = 2^63", "512 x 2^32", "min_size must be >= 1 (got %lld)",
                  "rows must be in 1..256 (got %d)", "no bflbm_ring_component_create", "derived, not measured", "18-connectivity",
                  "static LDS 24, 16, 64, 6144, 0, 43008 and 0 bytes", "a float sum per component has no fixed order"):
        assert words in block, words
    limits = re.sub(r"\s*\n//\s+", " ", open(os.path.join(CSRC, "bflbm_components.h")).read())
    for words in ("kHeader = 6", "kRowWords = 18", "kMaxRows = 256", "kLaunches = %d" % ks.LAUNCHES, "kMaxExtent = 65536", "derived, not measured",
                  "necessary for wrapping, not sufficient", "cluster_label_level", "cluster_resolve_level"):
        assert words in limits, words
    cluster = open(os.path.join(CSRC, "bflbm_cluster.h")).read()
    assert "bflbm_components.h" in cluster[cluster.index("// Out of scope"):cluster.index("// Host part")]


def test_component_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_longlong * 8)()
    levels = (ctypes.c_double * 1)(0.5)
    g = [ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()] + [ctypes.c_int() for _ in range(4)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 0, 1, levels, 0, 26, 1, 4, 1, 4, ctypes.byref(h))) for name in COMPONENT_SYMBOLS[:2]}
    calls.update({
        "bflbm_component_sample": lambda: lib.bflbm_component_sample(None),
        "bflbm_component_reset": lambda: lib.bflbm_component_reset(None),
        "bflbm_component_count": lambda: lib.bflbm_component_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_component_geometry": lambda: lib.bflbm_component_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_component_read": lambda: lib.bflbm_component_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null level array and a null result are refused before the handle is looked at
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in COMPONENT_SYMBOLS[:2]:
        assert getattr(lib, name)(owner, 0, 0, 1, None, 0, 26, 1, 4, 1, 4, ctypes.byref(h)) != 0
        assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 0, 1, levels, 0, 26, 1, 4, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_component_destroy(None) == 0          # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers -----------------------------------------------------------------------------------------
def test_refusals_rank_arc_and_brick_keys_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "component_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "component_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 21 + 7 * 6 * 2 * 2 * 3  # the checks component_main.cpp makes (21, then boxes x fills x connectivities x orders x pairs): one that silently stops running fails here


def test_the_helper_mirrors_the_geometry():
    assert ks.geometry(5, 26, 3, 16) == (5, 26, 3, 16, 6, 18, 9) and ks.LAUNCHES == cs.LAUNCHES - 1 + 6      # the labelling's three, six more
    assert ks.arcs([5, 6, 0, 1], 7) == [(5, 4)] and ks.arcs([0, 1, 2], 3) == [(0, 3)] and ks.arcs([1, 3], 5) == [(1, 1), (3, 1)] and ks.arcs([0], 1) == [(0, 1)]


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_component_kernel_metadata(device_asm):
    """Every k_component_* exists once: no scratch; the static LDS is what include/bflbm.h states.  The cluster trace's
    kernels, which the component trace launches, are still the six of tests/test_cluster_abi.py."""
    lds = {"k_component_count": 24, "k_component_scan": 16, "k_component_rank": 64, "k_component_masks": 6144, "k_component_origin": 0,
           "k_component_moments": 43008, "k_component_finish": 0}
    for name, want in lds.items():
        found = kernels(device_asm, mangled(name))
        assert len(found) == 1, (name, len(found))
        meta = found[0][1]
        assert re.search(r"; LDSByteSize: %d\b" % want, meta), f"{name}: LDS"
        assert re.search(r"; ScratchSize: 0\b", meta), f"{name} spills to scratch"
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_component_\w*:")) == len(lds)
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_cluster_\w*:")) == 6
