"""Morphology traces, CPU side: analysis.minkowski_counts against the set construction of tests/morph_counts.py (which
never forms an OR over a neighbourhood), the closed forms, the invariance under periodic shifts, the planted values,
the C-ABI surface (declared, exported, bound with the header's argument lists), the null-pointer refusals (which must
fail before any device is touched), the host part of csrc/bflbm_morph.h through a stand-alone program built with the
address and undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU
needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import morph_counts as mc
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

MORPH_SYMBOLS = ["bflbm_morph_create", "bflbm_batch_morph_create", "bflbm_morph_destroy", "bflbm_morph_sample", "bflbm_morph_reset",
                 "bflbm_morph_count", "bflbm_morph_geometry", "bflbm_morph_read"]
BOXES = [(7, 9, 5), (64, 32, 3), (6, 4, 1), (2, 2, 2), (1, 3, 2), (1, 1, 1), (33, 17, 6)]      # (nx, ny, nz)
FILLS = [0.05, 0.3, 0.5, 0.8, 1.0]


def _counts(pkg, occ):
    """The twin's counts of a boolean set: the field is the set itself, the level one half."""
    return tuple(int(v) for v in pkg.analysis.minkowski_counts(np.asarray(occ, dtype=np.float64), [0.5])[0])


# ---- the numpy twin against the set construction ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES)
def test_minkowski_counts_against_the_set_construction(pkg, n):
    nx, ny, nz = n
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    for fill in FILLS:
        v = rng.random((nz, ny, nx))
        got = pkg.analysis.minkowski_counts(v, [1.0 - fill, 2.0], "above")
        assert got.dtype == np.int64 and got.shape == (2, 4)
        assert tuple(got[0].tolist()) == mc.brute(v >= 1.0 - fill), (n, fill)
        assert got[1].tolist() == [0, 0, 0, 0]
        below = pkg.analysis.minkowski_counts(v, [fill], "below")
        assert tuple(below[0].tolist()) == mc.brute(v < fill), (n, fill)
        assert np.array_equal(pkg.analysis.minkowski_counts(v, [fill], 1), below)                 # the side by number
    sites = nx * ny * nz
    assert _counts(pkg, np.ones((nz, ny, nx))) == mc.brute(np.ones((nz, ny, nx))) == (sites, 3 * sites, 3 * sites, sites)


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def test_closed_forms(pkg):
    an = pkg.analysis
    n = (9, 8, 10)                                         # [nz, ny, nx]
    for a, b, c in ((1, 1, 1), (3, 2, 4), (8, 7, 9), (1, 5, 1)):
        occ = np.zeros(n, dtype=bool)
        occ[1:1 + a, 0:b, 0:c] = True                      # one empty cell at the least before the periodic image
        assert mc.functionals(_counts(pkg, occ)) == mc.cuboid(a, b, c), (a, b, c)
    full = np.ones(n, dtype=bool)
    assert mc.functionals(_counts(pkg, full)) == (720, 0, 0, 0)
    assert _counts(pkg, np.zeros(n)) == (0, 0, 0, 0)
    # two voxels that touch at a corner are one component (closed voxels: 26-connectivity of the set)
    pair = np.zeros(n, dtype=bool)
    pair[2, 2, 2] = pair[3, 3, 3] = True
    assert mc.functionals(_counts(pkg, pair)) == (2, 12, 6, 1)
    pair[3, 3, 3] = False; pair[6, 6, 6] = True           # apart: two components
    assert mc.functionals(_counts(pkg, pair)) == (2, 12, 6, 2)
    # a slab across two periodic directions: chi = 0, S = 2 nx ny; a rod along one: chi = 0
    slab = np.zeros(n, dtype=bool)
    slab[3:6] = True
    assert mc.functionals(_counts(pkg, slab)) == (3 * 80, 2 * 80, 0, 0)
    wrapped = np.roll(slab, 5, axis=0)                     # planes 8, 0, 1: across the periodic plane
    assert wrapped[0].all() and wrapped[8].all() and mc.functionals(_counts(pkg, wrapped)) == (240, 160, 0, 0)
    rod = np.zeros(n, dtype=bool)
    rod[2:4, 3:6, :] = True                                # 2 x 3 across, all of x
    assert mc.functionals(_counts(pkg, rod)) == (60, 2 * 10 * (2 + 3), 10, 0)
    # K separated voxels: chi = K
    many = np.zeros(n, dtype=bool)
    many[::3, ::3, ::3] = True                             # z 0 3 6, y 0 3 6 (8 wraps to 0 two apart), x 0 3 6 9 (9 next to 0!)
    many[:, :, 9] = False
    k = int(many.sum())
    assert k == 27 and mc.functionals(_counts(pkg, many)) == (k, 6 * k, 3 * k, k)
    # a voxelised sphere: one component without a tunnel or a cavity, S = 2 x the three projected areas
    z, y, x = np.indices((16, 16, 16))
    ball = (z - 7.5) ** 2 + (y - 7.5) ** 2 + (x - 7.5) ** 2 <= 5.3 ** 2
    assert mc.orthogonally_convex(ball)
    v, s, b2, chi = mc.functionals(_counts(pkg, ball))
    assert chi == 1 and v == int(ball.sum()) and s == 2 * sum(mc.projections(ball))
    f = an.minkowski_functionals(an.minkowski_counts(ball.astype(float), [0.5, 0.5]))
    assert f.dtype == np.int64 and f.tolist() == [[v, s, b2, chi]] * 2
    assert an.morphology_length(an.minkowski_counts(ball.astype(float), [0.5]), 4096).tolist() == [4096 / s]
    assert np.isnan(an.morphology_length(np.array([[720, 2160, 2160, 720]]), 720)).all()      # the full box: S = 0


@pytest.mark.parametrize("n", [(7, 9, 5), (6, 4, 1), (2, 2, 2)])
def test_invariance_under_periodic_shifts(pkg, n):
    nx, ny, nz = n
    rng = np.random.default_rng(5)
    v = rng.random((nz, ny, nx))
    want = pkg.analysis.minkowski_counts(v, [0.2, 0.5, 0.9])
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 5), (-1, -1, -1)):
        assert np.array_equal(pkg.analysis.minkowski_counts(np.roll(v, shift, axis=(0, 1, 2)), [0.2, 0.5, 0.9]), want), shift
    # the mirror image and a transposition of two equal-rule axes change no count either
    assert np.array_equal(pkg.analysis.minkowski_counts(v[::-1, ::-1, ::-1], [0.2, 0.5, 0.9]), want)
    assert np.array_equal(pkg.analysis.minkowski_counts(v.transpose(1, 0, 2), [0.2, 0.5, 0.9]), want)


def test_planted_values(pkg):
    """A site equal to the level is occupied above and not below; -0.0 equals +0.0 either way round; +inf is above every
    finite level, -inf below; a NaN occupies nothing on either side."""
    an = pkg.analysis
    big = np.finfo(np.float64).max
    v = np.full((4, 4, 4), 0.25)
    v[1, 1, 1] = 0.5
    assert an.minkowski_counts(v, [0.5], "above")[0].tolist() == [1, 6, 12, 8]
    assert an.minkowski_counts(v, [0.5], "below")[0, 0] == 63
    for zero, level in ((0.0, -0.0), (-0.0, 0.0)):
        v = np.full((4, 4, 4), -1.0)
        v[2, 2, 2] = zero
        assert an.minkowski_counts(v, [level], "above")[0].tolist() == [1, 6, 12, 8]
        assert an.minkowski_counts(v, [level], "below")[0, 0] == 63
    v = np.zeros((4, 4, 4))
    v[0, 0, 0], v[3, 3, 3], v[1, 2, 3] = np.inf, -np.inf, np.nan
    assert an.minkowski_counts(v, [big, -big], "above")[:, 0].tolist() == [1, 62]
    assert an.minkowski_counts(v, [big, -big], "below")[:, 0].tolist() == [62, 1]
    assert an.minkowski_counts(np.full((3, 3, 3), np.nan), [0.0], "above").tolist() == [[0, 0, 0, 0]]
    assert an.minkowski_counts(np.full((3, 3, 3), np.nan), [0.0], "below").tolist() == [[0, 0, 0, 0]]
    # both sides of a field without NaN are complements: the volumes add up to the box
    v = np.random.default_rng(3).random((5, 6, 7))
    assert an.minkowski_counts(v, [0.4])[0, 0] + an.minkowski_counts(v, [0.4], "below")[0, 0] == 210


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((3, 4, 5))
    for bad in (lambda: an.minkowski_counts(f[0], [0.0]), lambda: an.minkowski_counts(f, []), lambda: an.minkowski_counts(f, [0.0] * 9),
                lambda: an.minkowski_counts(f, [np.nan]), lambda: an.minkowski_counts(f, [0.0, np.inf]), lambda: an.minkowski_counts(f, [0.0], "left"),
                lambda: an.minkowski_counts(f, [0.0], 2), lambda: an.minkowski_counts(f, [[0.0]]), lambda: an.minkowski_counts(np.zeros((0, 4, 5)), [0.0]),
                lambda: an.minkowski_functionals(np.zeros((2, 3), dtype=np.int64)), lambda: an.minkowski_functionals(np.zeros((2, 4)))):
        with pytest.raises(ValueError):
            bad()
    assert an.minkowski_counts(f, 0.0).shape == (1, 4) and an.minkowski_counts(f, [0.0] * 8).shape == (8, 4)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_morph_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in MORPH_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_morph_create"] == sig["bflbm_batch_morph_create"]
    # (owner, source, var, nlevels, levels, side, every, capacity, out)
    assert len(sig["bflbm_morph_create"][1]) == 9 and sig["bflbm_morph_create"][1][7] is ctypes.c_longlong
    assert sig["bflbm_morph_read"][1][3] == ctypes.POINTER(ctypes.c_longlong)          # integers, not doubles
    assert len(sig["bflbm_morph_geometry"][1]) == 6
    assert header.count("Morphology traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert "bflbm_ring_morph_create" not in sig and not hasattr(lib, "bflbm_ring_morph_create")      # a ring is out of scope
    assert hasattr(pkg, "MorphologyTrace") and "MorphologyTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "morphology_trace")
    assert not hasattr(pkg.RingLBM, "morphology_trace")
    for fn in ("minkowski_counts", "minkowski_functionals", "morphology_length"):
        assert hasattr(pkg.analysis, fn)
    # the header, the numpy twin and the tests' helper state the same constants
    assert pkg.analysis.MORPH_MAX_LEVELS == 8 and pkg.analysis.MORPH_SIDES == pkg.lattice.MORPH_SIDES == {"above": 0, "below": 1}
    block = header[header.index("Morphology traces:"):header.index("typedef struct bflbm_morph")]
    for words in ("nlevels in 1..8", "tile of %d consecutive plane sites" % mc.TILE, "largest of 64, 32, 16, 8", "%d work items" % mc.WANT_ITEMS,
                  "S = -6 N3 + 2 N2", "2B = 3 N3 - 2 N2 + N1", "chi = -N3 + N2 - N1 + N0", "no bflbm_ring_morph_create", "at most 3 to a counter"):
        assert words in block, words


def test_morph_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_longlong * 8)()
    levels = (ctypes.c_double * 1)(0.5)
    g = [ctypes.c_int() for _ in range(5)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 0, 1, levels, 0, 1, 4, ctypes.byref(h))) for name in MORPH_SYMBOLS[:2]}
    calls.update({
        "bflbm_morph_sample": lambda: lib.bflbm_morph_sample(None),
        "bflbm_morph_reset": lambda: lib.bflbm_morph_reset(None),
        "bflbm_morph_count": lambda: lib.bflbm_morph_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_morph_geometry": lambda: lib.bflbm_morph_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_morph_read": lambda: lib.bflbm_morph_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null level array and a null result are refused before the owner is looked at: any non-null pointer will do
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in MORPH_SYMBOLS[:2]:
        assert getattr(lib, name)(owner, 0, 0, 1, None, 0, 1, 4, ctypes.byref(h)) != 0
        assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 0, 1, levels, 0, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_morph_destroy(None) == 0              # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_levels_launch_shape_and_refusals_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "morph_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "morph_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 26  # the checks morph_main.cpp makes: a check that silently stops running fails here


def test_the_helper_mirrors_the_launch_shape():
    """tests/morph_counts.geometry against the figures morph_main.cpp holds the host part to."""
    assert mc.geometry((7, 9, 5), 3) == (3, 1024, 5, 1, 1) and mc.geometry((7, 9, 19), 1) == (1, 1024, 8, 3, 3)
    assert mc.geometry((256, 256, 256), 3) == (3, 1024, 16, 1024, 1024) and mc.geometry((64, 64, 64), 3, 16) == (3, 1024, 8, 32, 512)
    assert mc.geometry((1024, 1024, 1024), 8) == (8, 1024, 64, 16384, 16384) and mc.geometry((70, 30, 19), 2, 3) == (2, 1024, 8, 9, 27)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_morph_kernel_metadata(device_asm):
    """k_morph_count<NL>, NL = 1 .. 8: no scratch, no dynamic LDS; the static LDS is the 32 counters of 4 bytes that
    include/bflbm.h states.  The finishing launch is k_hist_finish, which test_hist_abi.py checks."""
    found = kernels(device_asm, r"^_Z\w*?13k_morph_countILi(\d)EE\w*:")      # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        assert re.search(r"; LDSByteSize: 128\b", meta), f"{m.group(0)}: LDS"
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
    assert len(kernels(device_asm, r"^_Z\w*?13k_hist_finish(E)\w*:")) == 1      # one finishing kernel, shared
