"""Cluster traces, CPU side: analysis.cluster_labels and analysis.cluster_record against the flood fill of
tests/cluster_sets.py (which never propagates a minimum), the closed forms, the invariances, the record's identities, the
planted values, the C-ABI surface (declared, exported, bound with the header's argument lists), the null-pointer refusals
(which must fail before any device is touched), the host part of csrc/bflbm_cluster.h and the find and union functions
the kernels instantiate through a stand-alone program built with the address and undefined-behaviour sanitizers, and the
compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels, mangled   # noqa: F401  (device_asm: the listing fixture)

import cluster_sets as cs
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

CLUSTER_SYMBOLS = ["bflbm_cluster_create", "bflbm_batch_cluster_create", "bflbm_cluster_destroy", "bflbm_cluster_sample", "bflbm_cluster_reset",
                   "bflbm_cluster_count", "bflbm_cluster_geometry", "bflbm_cluster_read", "bflbm_cluster_labels"]
BOXES = [(7, 9, 5), (64, 32, 3), (6, 4, 1), (2, 2, 2), (1, 3, 2), (1, 1, 1), (33, 17, 6)]      # (nx, ny, nz)
FILLS = [0.05, 0.1, 0.31, 0.5, 0.8, 1.0]


def _labels(pkg, occ, connectivity):
    """The twin's labels of a boolean set: the field is the set itself, the level one half."""
    return pkg.analysis.cluster_labels(np.asarray(occ, dtype=np.float64), 0.5, "above", connectivity)


def _record(pkg, occ, connectivity):
    return pkg.analysis.cluster_record(np.asarray(occ, dtype=np.float64), [0.5], "above", connectivity)[0].tolist()


# ---- the numpy twin against the flood fill -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES)
def test_cluster_labels_against_the_flood_fill(pkg, n):
    nx, ny, nz = n
    an = pkg.analysis
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    for fill in FILLS:
        v = rng.random((nz, ny, nx))
        for connectivity in cs.CONNECTIVITIES:
            for side, level, occ in (("above", 1.0 - fill, v >= 1.0 - fill), ("below", fill, v < fill)):
                want = cs.flood(occ, connectivity)
                got = an.cluster_labels(v, level, side, connectivity)
                assert got.dtype == np.int32 and got.shape == (nz, ny, nx)
                assert np.array_equal(got, want), (n, fill, side, connectivity)
                rec = an.cluster_record(v, [level, 2.0 if side == "above" else -1.0], side, connectivity)
                assert rec.dtype == np.int64 and rec.shape == (2, cs.WORDS)
                assert rec[0].tolist() == cs.record(want), (n, fill, side, connectivity)
                assert rec[1].tolist() == [0, 0, 0, -1] + [0] * 34                                 # nothing occupied
                assert np.array_equal(an.cluster_labels(v, level, {"above": 0, "below": 1}[side], connectivity), got)   # the side by number
                roots, sizes = an.cluster_sizes(got)
                assert len(roots) == rec[0, 0] and sizes.sum() == rec[0, 1] == occ.sum() and (got.ravel()[roots] == roots).all()


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def test_closed_forms(pkg):
    n = (9, 8, 10)                                         # [nz, ny, nx]
    sites = 720
    for c in cs.CONNECTIVITIES:
        assert _record(pkg, np.zeros(n), c) == [0, 0, 0, -1] + [0] * 34 and (_labels(pkg, np.zeros(n), c) == -1).all()
        full = _record(pkg, np.ones(n), c)                 # one component of nsites: 512 <= 720 < 1024
        assert full[:6] == [1, sites, sites, 0, sites * sites, 0] and full[6 + 9] == 1 and sum(full[6:]) == 1
        assert (_labels(pkg, np.ones(n), c) == 0).all()
        # K separated voxels
        many = np.zeros(n, dtype=bool)
        many[::3, ::3, ::3] = True                         # z 0 3 6, y 0 3 6, x 0 3 6 9 (9 next to 0 across the wrap)
        many[:, :, 9] = False
        k = int(many.sum())
        rec = _record(pkg, many, c)
        assert k == 27 and rec[:6] == [k, k, 1, 0, k, 0] and rec[6] == k
        # two voxels that touch at a corner: one component under 26, two under 6
        pair = np.zeros(n, dtype=bool)
        pair[2, 2, 2] = pair[3, 3, 3] = True
        first = (2 * 8 + 2) * 10 + 2
        assert _record(pkg, pair, c)[:5] == ([1, 2, 2, first, 4] if c == 26 else [2, 2, 1, first, 2])
        # a diagonal staircase of corner-touching voxels, across the periodic corner too on a cube
        stairs = np.zeros((6, 6, 6), dtype=bool)
        for i in range(6):
            stairs[i, i, i] = True
        assert _record(pkg, stairs, c)[:5] == ([1, 6, 6, 0, 36] if c == 26 else [6, 6, 1, 0, 6])
        # a slab wrapped across the periodic plane is one component, two slabs are two
        slab = np.zeros(n, dtype=bool)
        slab[[8, 0, 1]] = True
        assert _record(pkg, slab, c)[:5] == [1, 240, 240, 0, 240 * 240]
        lab = _labels(pkg, slab, c)
        assert (lab[[8, 0, 1]] == 0).all() and (lab[2:8] == -1).all()
        slab[4:6] = True
        assert _record(pkg, slab, c)[:5] == [2, 400, 240, 0, 240 * 240 + 160 * 160]
        assert (_labels(pkg, slab, c)[4:6] == 4 * 80).all()
        # a voxelised ball: one component, its label its first site
        z, y, x = np.indices((16, 16, 16))
        ball = (z - 7.5) ** 2 + (y - 7.5) ** 2 + (x - 7.5) ** 2 <= 5.3 ** 2
        rec = _record(pkg, ball, c)
        first = int(np.flatnonzero(ball.ravel())[0])
        assert rec[:5] == [1, int(ball.sum()), int(ball.sum()), first, int(ball.sum()) ** 2]
    # a 3-D checkerboard on even extents: nsites / 2 singletons under 6, one component under 26
    z, y, x = np.indices((4, 6, 8))
    board = (z + y + x) % 2 == 0
    assert _record(pkg, board, 6)[:7] == [96, 96, 1, 0, 96, 0, 96]
    assert _record(pkg, board, 26)[:5] == [1, 96, 96, 0, 96 * 96]
    # the helper's snake: one component under both connectivities whose label is its end
    snake = cs.snake((19, 31, 34))
    for c in cs.CONNECTIVITIES:
        assert _record(pkg, snake, c)[:4] == [1, int(snake.sum()), int(snake.sum()), 0] and snake.sum() > 2000
        assert np.array_equal(_labels(pkg, snake, c), cs.flood(snake, c))


# ---- invariances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(7, 9, 5), (6, 4, 1), (2, 2, 2)])
def test_invariance_under_shifts_mirrors_and_transpositions(pkg, n):
    nx, ny, nz = n
    an = pkg.analysis
    v = np.random.default_rng(5).random((nz, ny, nx))
    levels = [0.2, 0.5, 0.9]
    for c in cs.CONNECTIVITIES:
        want = an.cluster_record(v, levels, "above", c)
        parts = {frozenset(g) for g in cs.canonical(an.cluster_labels(v, 0.5, "above", c)).values()}
        for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 5), (-1, -1, -1)):
            moved = np.roll(v, shift, axis=(0, 1, 2))
            rec = an.cluster_record(moved, levels, "above", c)
            assert np.array_equal(np.delete(rec, 3, axis=1), np.delete(want, 3, axis=1)), shift       # word 3 is a position
            back = {frozenset(((z - shift[0]) % nz, (y - shift[1]) % ny, (x - shift[2]) % nx) for z, y, x in g)
                    for g in cs.canonical(an.cluster_labels(moved, 0.5, "above", c)).values()}
            assert back == parts, shift                    # the same sets of sites, whatever their labels
        for image in (v[::-1, ::-1, ::-1], v.transpose(1, 0, 2), v.transpose(2, 1, 0)):
            rec = an.cluster_record(image, levels, "above", c)
            assert np.array_equal(np.delete(rec, 3, axis=1), np.delete(want, 3, axis=1))


# ---- the identities of a record -------------------------------------------------------------------------------------------------
def test_record_identities(pkg):
    an = pkg.analysis
    v = np.random.default_rng(11).random((19, 31, 34))
    levels = [0.05, 0.1, 0.31, 0.5, 0.9]
    for c in cs.CONNECTIVITIES:
        rec = an.cluster_record(v, levels, "below", c)
        counts = an.minkowski_counts(v, levels, "below")
        for l, level in enumerate(levels):
            ncomp, vol, smax, label, s2, capped = rec[l, :6].tolist()
            assert rec[l, 6:].sum() == ncomp and vol == counts[l, 0] and capped == 0
            assert smax * smax <= s2 <= vol * vol
            roots, sizes = an.cluster_sizes(an.cluster_labels(v, level, "below", c))
            assert label == roots[sizes == smax].min() and smax == sizes.max() and s2 == (sizes ** 2).sum()
            for b in range(32):
                assert rec[l, 6 + b] == np.count_nonzero((sizes >= 2 ** b) & (sizes < 2 ** (b + 1)))
    assert (an.cluster_record(v, levels, "below", 6)[:, 0] >= an.cluster_record(v, levels, "below", 26)[:, 0]).all()


def test_planted_values(pkg):
    """A site equal to the level is occupied above and not below; -0.0 equals +0.0 either way round; +inf is above every
    finite level, -inf below; a NaN occupies nothing on either side."""
    an = pkg.analysis
    big = np.finfo(np.float64).max
    v = np.full((4, 4, 4), 0.25)
    v[1, 1, 1] = 0.5
    assert an.cluster_record(v, [0.5], "above")[0, :5].tolist() == [1, 1, 1, 21, 1]
    assert an.cluster_record(v, [0.5], "below")[0, :5].tolist() == [1, 63, 63, 0, 63 * 63]
    assert an.cluster_labels(v, 0.5, "below")[1, 1, 1] == -1
    for zero, level in ((0.0, -0.0), (-0.0, 0.0)):
        v = np.full((4, 4, 4), -1.0)
        v[2, 2, 2] = zero
        assert an.cluster_record(v, [level], "above")[0, :4].tolist() == [1, 1, 1, 42]
        assert an.cluster_record(v, [level], "below")[0, :4].tolist() == [1, 63, 63, 0]
    v = np.zeros((4, 4, 4))
    v[0, 0, 0], v[3, 3, 3], v[1, 2, 3] = np.inf, -np.inf, np.nan
    assert an.cluster_record(v, [big, -big], "above")[:, :4].tolist() == [[1, 1, 1, 0], [1, 62, 62, 0]]
    assert an.cluster_record(v, [big, -big], "below")[:, :4].tolist() == [[1, 62, 62, 1], [1, 1, 1, 63]]
    for side in ("above", "below"):
        assert an.cluster_record(np.full((3, 3, 3), np.nan), [0.0], side)[0, :4].tolist() == [0, 0, 0, -1]
        assert (an.cluster_labels(v, 0.0, side)[1, 2, 3] == -1)


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((3, 4, 5))
    for bad in (lambda: an.cluster_record(f[0], [0.0]), lambda: an.cluster_record(f, []), lambda: an.cluster_record(f, [0.0] * 9),
                lambda: an.cluster_record(f, [np.nan]), lambda: an.cluster_record(f, [0.0, np.inf]), lambda: an.cluster_record(f, [0.0], "left"),
                lambda: an.cluster_record(f, [0.0], 2), lambda: an.cluster_record(f, [[0.0]]), lambda: an.cluster_record(np.zeros((0, 4, 5)), [0.0]),
                lambda: an.cluster_record(f, [0.0], "above", 18), lambda: an.cluster_labels(f, 0.0, "above", 8), lambda: an.cluster_labels(f, [0.0, 1.0]),
                lambda: an.cluster_labels(f, np.nan), lambda: an.cluster_sizes(np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            bad()
    assert an.cluster_record(f, 0.0).shape == (1, 38) and an.cluster_record(f, [0.0] * 8, "below", 6).shape == (8, 38)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_cluster_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in CLUSTER_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_cluster_create"] == sig["bflbm_batch_cluster_create"]
    # (owner, source, var, nlevels, levels, side, connectivity, every, capacity, out)
    assert len(sig["bflbm_cluster_create"][1]) == 10 and sig["bflbm_cluster_create"][1][8] is ctypes.c_longlong
    assert sig["bflbm_cluster_read"][1][3] == ctypes.POINTER(ctypes.c_longlong)          # integers, not doubles
    assert sig["bflbm_cluster_labels"][1][2] == ctypes.POINTER(ctypes.c_int)            # 32-bit labels
    assert len(sig["bflbm_cluster_geometry"][1]) == 8
    assert header.count("Cluster traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert "bflbm_ring_cluster_create" not in sig and not hasattr(lib, "bflbm_ring_cluster_create")      # a ring is out of scope
    assert hasattr(pkg, "ClusterTrace") and "ClusterTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "cluster_trace")
    assert not hasattr(pkg.RingLBM, "cluster_trace")
    for fn in ("cluster_labels", "cluster_record", "cluster_sizes"):
        assert hasattr(pkg.analysis, fn)
    for method in ("read", "components", "largest", "size_histogram", "mean_sizes", "labels", "geometry", "names"):
        assert hasattr(pkg.ClusterTrace, method)
    # the header, the numpy twin, the tests' helper and the kernels' header state the same constants
    assert pkg.analysis.CLUSTER_WORDS == cs.WORDS == 38 and tuple(pkg.analysis.CLUSTER_CONNECTIVITIES) == cs.CONNECTIVITIES == (6, 26)
    block = re.sub(r"\s*\n \*\s+", " ", header[header.index("Cluster traces:"):header.index("typedef struct bflbm_cluster")])
    for words in ("nlevels in 1..8", "W = %d" % cs.WORDS, "brick of %d x %d x %d sites" % cs.BRICK, "(%d, %d, %d)" % cs.BRICK,
                  "the launches per level (%d)" % cs.LAUNCHES, "then per level, one after another", "%d launches: k_cluster_local" % cs.LAUNCHES,
                  "connectivity must be 6 or 26 (got %d)", "no bflbm_ring_cluster_create", "nx ny nz > 2^31 - 1",
                  "(size << 32) | (0xffffffff - label)", "word 6 + b", "static LDS 4096 bytes", "152 bytes", "18-connectivity"):
        assert words in block, words
    limits = open(os.path.join(CSRC, "bflbm_cluster.h")).read()
    for words in ("kWords = 38", "kBins = 32, kFirstBin = 6", "kBx = %d, kBy = %d, kBz = %d" % cs.BRICK, "kLaunches = %d" % cs.LAUNCHES,
                  "kMaxSites = 2147483647LL", "no bflbm_ring_cluster_create"):
        assert words in limits, words


def test_cluster_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_longlong * 8)()
    ints = (ctypes.c_int * 8)()
    levels = (ctypes.c_double * 1)(0.5)
    g = [ctypes.c_int() for _ in range(7)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 0, 1, levels, 0, 26, 1, 4, ctypes.byref(h))) for name in CLUSTER_SYMBOLS[:2]}
    calls.update({
        "bflbm_cluster_sample": lambda: lib.bflbm_cluster_sample(None),
        "bflbm_cluster_reset": lambda: lib.bflbm_cluster_reset(None),
        "bflbm_cluster_count": lambda: lib.bflbm_cluster_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_cluster_geometry": lambda: lib.bflbm_cluster_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_cluster_read": lambda: lib.bflbm_cluster_read(None, 0, 1, buf, None),
        "bflbm_cluster_labels": lambda: lib.bflbm_cluster_labels(None, 0, ints),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null level array, a null result and a null label array are refused before the handle is looked at
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in CLUSTER_SYMBOLS[:2]:
        assert getattr(lib, name)(owner, 0, 0, 1, None, 0, 26, 1, 4, ctypes.byref(h)) != 0
        assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 0, 1, levels, 0, 26, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_cluster_labels(owner, 0, None) != 0 and "bflbm_cluster_labels: null" in lib.bflbm_last_error().decode()
    assert lib.bflbm_cluster_destroy(None) == 0            # like every destroy of the ABI: nothing to do


# ---- the host part and the algorithm under the sanitizers -------------------------------------------------------------------
def test_refusals_geometry_and_the_sequential_union_find_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "cluster_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "cluster_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 22 + 7 * 6 * 2 * 3  # the checks cluster_main.cpp makes (22, then boxes x fills x connectivities x orders): one that silently stops running fails here


def test_the_helper_mirrors_the_geometry():
    """tests/cluster_sets.geometry against the figures cluster_main.cpp holds the host part to."""
    assert cs.bricks((7, 9, 5)) == 6 and cs.bricks((32, 4, 4)) == 1 and cs.bricks((34, 31, 19)) == 80 and cs.bricks((70, 30, 6)) == 48
    assert cs.bricks((256, 256, 256)) == 32768 and cs.geometry((34, 31, 19), 5, 26) == (5, 26, 32, 4, 4, 80, 4)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_cluster_kernel_metadata(device_asm):
    """Every k_cluster_* exists once: no scratch; the static LDS is what include/bflbm.h states: 4096 bytes for the
    brick's parents and counts, 152 for the workgroup's sums, none elsewhere."""
    lds = {"k_cluster_local": 4096, "k_cluster_merge": 0, "k_cluster_resolve": 0, "k_cluster_stats": 152, "k_cluster_finish": 0,
           "k_cluster_flatten": 0}
    for name, want in lds.items():
        found = kernels(device_asm, mangled(name))
        assert len(found) == 1, (name, len(found))
        meta = found[0][1]
        assert re.search(r"; LDSByteSize: %d\b" % want, meta), f"{name}: LDS"
        assert re.search(r"; ScratchSize: 0\b", meta), f"{name} spills to scratch"
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_cluster_\w*:")) == len(lds)
