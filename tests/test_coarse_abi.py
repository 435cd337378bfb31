"""Coarse traces, CPU side: analysis.coarse_fields against the site-by-site walk of tests/coarse_blocks.py (which shares no
construction with it), the closed forms, the refusals of the twin, the C-ABI surface (declared, exported, bound with the
header's argument lists), the null-pointer refusals (which must fail before any device is touched), the host part of
csrc/bflbm_coarse.h through a stand-alone program built with the address and undefined-behaviour sanitizers, the compiled
kernels' metadata (hipcc cross-compiles gfx950, no GPU needed) and the plotfiles of a synthetic record."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import coarse_blocks as cb
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

COARSE_SYMBOLS = ["bflbm_coarse_create", "bflbm_batch_coarse_create", "bflbm_coarse_destroy", "bflbm_coarse_sample", "bflbm_coarse_reset",
                  "bflbm_coarse_count", "bflbm_coarse_geometry", "bflbm_coarse_read"]
PAIRS = [(0, 1), (2, 2)]


def _fields(case, nv=3):
    n = case[0]
    rng = np.random.default_rng(1000 * n[0] + 10 * n[1] + n[2])
    return rng.standard_normal((nv, n[2], n[1], n[0])) + 1.5


# ---- the numpy twin against the walk ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cb.CASES, ids=cb.case_id)
def test_coarse_fields_against_the_walk(pkg, case):
    n, origin, extent, block = case
    f = _fields(case)
    got = pkg.analysis.coarse_fields(f, PAIRS, origin, extent, block)
    want = np.array(cb.walk(f.tolist(), PAIRS, origin, extent, block))
    assert got.dtype == np.float64 and got.shape == (5,) + tuple(w // b for w, b in zip(extent[::-1], block[::-1]))
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert np.array_equal(pkg.analysis.coarse_fields(f[:1], [], origin, extent, block)[0], got[0])      # no pairs; one variable
    # the same blocks gathered by plain slicing of the rolled field: an exact permutation, summed to rounding only
    rolled = np.roll(f, [-origin[2], -origin[1], -origin[0]], axis=(1, 2, 3))[:, :extent[2], :extent[1], :extent[0]]
    cz, cy, cx = got.shape[1:]
    blocks = rolled.reshape(3, cz, block[2], cy, block[1], cx, block[0]).sum(axis=(2, 4, 6))
    sites = block[0] * block[1] * block[2]
    assert np.abs(got[:3] - blocks).max() <= sites * 2.0 ** -52 * np.abs(rolled).reshape(3, cz, block[2], cy, block[1], cx, block[0]).sum(axis=(2, 4, 6)).max()


def test_eight_variables_and_sixteen_pairs_against_the_walk(pkg):
    case = cb.CASES[2]                                     # the seam on all three axes
    n, origin, extent, block = case
    f = _fields(case, nv=8)
    pairs = [(k % 8, (3 * k) % 8) for k in range(16)]
    got = pkg.analysis.coarse_fields(f, pairs, origin, extent, block)
    assert got.shape[0] == 24 and np.array_equal(got, np.array(cb.walk(f.tolist(), pairs, origin, extent, block)))


# ---- the closed forms ---------------------------------------------------------------------------------------------------------
def test_closed_forms(pkg):
    an = pkg.analysis
    for n, origin, extent, block in cb.CASES:
        ones = np.ones((2, n[2], n[1], n[0]))
        got = an.coarse_fields(ones, [(0, 1)], origin, extent, block)
        assert (got == float(block[0] * block[1] * block[2])).all()        # a field of ones: the sites of a block everywhere
    f = _fields(cb.CASES[1])
    assert np.array_equal(an.coarse_fields(f), f) and np.array_equal(an.coarse_fields(f, block=(1, 1, 1), extent=(10, 6, 13)), f)      # block 1, full window
    assert np.array_equal(an.coarse_fields(f, [(1, 2)])[3], f[1] * f[2])
    # a window through the seam equals the same window of the rolled field
    for origin, extent, block in (((8, 5, 11), (6, 4, 6), (3, 2, 3)), ((9, 0, 0), (10, 6, 13), (2, 3, 13)), ((0, 3, 12), (5, 6, 2), (5, 1, 2))):
        rolled = np.roll(f, [-origin[2], -origin[1], -origin[0]], axis=(1, 2, 3))
        assert np.array_equal(an.coarse_fields(f, PAIRS, origin, extent, block), an.coarse_fields(rolled, PAIRS, (0, 0, 0), extent, block))
    # extent None: from the origin to the end of the box
    assert np.array_equal(an.coarse_fields(f, origin=(4, 0, 1), block=(3, 2, 4)), an.coarse_fields(f, origin=(4, 0, 1), extent=(6, 6, 12), block=(3, 2, 4)))
    # a NaN stays in its block
    g = f.copy()
    g[0, 7, 2, 3] = np.nan
    got = an.coarse_fields(g, [(0, 1)], (0, 0, 1), (10, 6, 12), (5, 3, 4))
    bad = np.isnan(got)
    assert bad.sum() == 2 and bad[0, 1, 0, 0] and bad[3, 1, 0, 0]
    # the block variance: the mean of the product minus the product of the means
    s = an.coarse_fields(f, [(0, 0), (0, 1)], block=(5, 3, 13))
    var = an.coarse_block_variance(s[0], s[0], s[3], 5 * 3 * 13)
    want = f[0].reshape(1, 13, 2, 3, 2, 5).var(axis=(1, 3, 5))
    assert var.shape == (1, 2, 2) and np.allclose(var, want, rtol=1e-12, atol=1e-13)
    cov = an.coarse_block_variance(s[0], s[1], s[4], 195)
    x, y = f[0].reshape(1, 13, 2, 3, 2, 5), f[1].reshape(1, 13, 2, 3, 2, 5)
    assert np.allclose(cov, (x * y).mean(axis=(1, 3, 5)) - x.mean(axis=(1, 3, 5)) * y.mean(axis=(1, 3, 5)), rtol=1e-12, atol=1e-13)


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((2, 13, 6, 10))
    for bad in (lambda: an.coarse_fields(f[0]), lambda: an.coarse_fields(np.zeros((9, 2, 2, 2))), lambda: an.coarse_fields(np.zeros((0, 2, 2, 2))),
                lambda: an.coarse_fields(np.zeros((1, 0, 2, 2))),
                lambda: an.coarse_fields(f, [(0, 0)] * 17), lambda: an.coarse_fields(f, [(0, 2)]), lambda: an.coarse_fields(f, [(-1, 0)]),
                lambda: an.coarse_fields(f, origin=(10, 0, 0)), lambda: an.coarse_fields(f, origin=(0, -1, 0)), lambda: an.coarse_fields(f, origin=(0, 0)),
                lambda: an.coarse_fields(f, origin=5),
                lambda: an.coarse_fields(f, extent=(11, 6, 13)), lambda: an.coarse_fields(f, extent=(10, 0, 13)), lambda: an.coarse_fields(f, extent=(10, 6, 14)),
                lambda: an.coarse_fields(f, block=(3, 1, 1)), lambda: an.coarse_fields(f, block=(1, 4, 1)), lambda: an.coarse_fields(f, block=(1, 1, 2)),
                lambda: an.coarse_fields(f, block=(0, 1, 1)), lambda: an.coarse_fields(f, block=(1, 1)),
                lambda: an.coarse_fields(np.zeros((1, 1, 1, 514)), block=(257, 1, 1)),
                lambda: an.coarse_block_variance(np.zeros(3), np.zeros(4), np.zeros(3), 8), lambda: an.coarse_block_variance(np.zeros(3), np.zeros(3), np.zeros(3), 0)):
        with pytest.raises(ValueError):
            bad()
    assert an.coarse_fields(np.zeros((8, 1, 1, 512)), [(0, 0)] * 16, block=(256, 1, 1)).shape == (24, 1, 1, 2)      # the limits themselves
    assert (an.COARSE_MAX_VARS, an.COARSE_MAX_PAIRS, an.COARSE_MAX_BLOCK_X) == (8, 16, cb.THREADS)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_coarse_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in COARSE_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_coarse_create"] == sig["bflbm_batch_coarse_create"]
    # (owner, source, nvars, vars, npairs, pair_a, pair_b, origin, extent, block, every, capacity, out)
    assert len(sig["bflbm_coarse_create"][1]) == 13 and sig["bflbm_coarse_create"][1][11] is ctypes.c_longlong
    assert sig["bflbm_coarse_read"][1][3] is ctypes.c_void_p                            # doubles
    assert len(sig["bflbm_coarse_geometry"][1]) == 8
    assert header.count("Coarse traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert "bflbm_ring_coarse_create" not in sig and not hasattr(lib, "bflbm_ring_coarse_create")      # a ring is out of scope
    assert hasattr(pkg, "CoarseTrace") and "CoarseTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "coarse_trace")
    assert not hasattr(pkg.RingLBM, "coarse_trace")
    for fn in ("coarse_fields", "coarse_block_variance"):
        assert hasattr(pkg.analysis, fn)
    # the header states the rule, the limits and what is not built; the kernel's header says why there is no ring
    block = header[header.index("Coarse traces:"):header.index("typedef struct bflbm_coarse")]
    for words in ("nvars in 1..8", "npairs in 0..16", "(o_a + i) mod n_a", "b_x <= 256", "c_a = w_a / b_a", "C = C + term", "S = S + C(d_x)",
                  "A NaN stays in its block", "[replica][Q][c_z][c_y][c_x]", "floor(256 / b_x) b_x", "%d / replicas" % cb.GROUPS,
                  "no bflbm_ring_coarse_create", "a block may straddle two slabs", "No scratch", "no static LDS", "no merge pass",
                  "8 nvars bytes read per window site"):
        assert words in block, words
    kernel_header = open(os.path.join(CSRC, "bflbm_coarse.h")).read()
    assert "a block may straddle two slabs" in kernel_header and "no bflbm_ring_coarse_create" in kernel_header


def test_coarse_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 16)()
    va, three = (ctypes.c_int * 1)(0), (ctypes.c_int * 3)(1, 1, 1)
    zero = (ctypes.c_int * 3)(0, 0, 0)
    g = [ctypes.c_int() for _ in range(7)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 1, va, 0, None, None, zero, three, three, 1, 4, ctypes.byref(h))) for name in COARSE_SYMBOLS[:2]}
    calls.update({
        "bflbm_coarse_sample": lambda: lib.bflbm_coarse_sample(None),
        "bflbm_coarse_reset": lambda: lib.bflbm_coarse_reset(None),
        "bflbm_coarse_count": lambda: lib.bflbm_coarse_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_coarse_geometry": lambda: lib.bflbm_coarse_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_coarse_read": lambda: lib.bflbm_coarse_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null array and a null result are refused before the owner is looked at: any non-null pointer will do
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in COARSE_SYMBOLS[:2]:
        for args in ((None, 0, None, None, zero, three, three), (va, 0, None, None, None, three, three), (va, 0, None, None, zero, None, three),
                     (va, 0, None, None, zero, three, None)):
            assert getattr(lib, name)(owner, 0, 1, *args, 1, 4, ctypes.byref(h)) != 0
            assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 1, va, 0, None, None, zero, three, three, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_coarse_destroy(None) == 0             # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_window_refusals_and_launch_shapes_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "coarse_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "coarse_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 295  # the checks coarse_main.cpp makes: a check that silently stops running fails here


def test_the_helper_mirrors_the_launch_shape():
    """tests/coarse_blocks.geometry against the figures coarse_main.cpp holds the host part to."""
    want = [(4, 4, 4, 5, 256, 16, 4), (2, 2, 3, 5, 255, 6, 2), (2, 2, 2, 5, 255, 4, 1), (10, 6, 1, 5, 256, 6, 2), (10, 3, 8, 5, 252, 24, 12),
            (86, 4, 2, 5, 255, 16, 16), (4, 3, 2, 5, 195, 12, 12), (520, 2, 2, 5, 256, 12, 12), (2, 1, 2, 5, 256, 4, 4)]
    assert [cb.geometry(extent, block, 5) for _, _, extent, block in cb.CASES] == want
    assert cb.geometry((256, 256, 256), (4, 4, 4), 3) == (64, 64, 64, 3, 256, 4096, 2048) and cb.geometry((256, 256, 1), (1, 1, 1), 3)[5:] == (256, 256)
    assert cb.geometry((64, 64, 64), (2, 2, 2), 3, 16) == (32, 32, 32, 3, 256, 1024, 2048) and cb.geometry((8, 8, 8), (2, 2, 2), 1, 4096)[6] == 4096
    assert cb.geometry((6, 4, 6), (3, 2, 3), 5, 3)[5:] == (4, 3) and all(cb.tile(b) % b == 0 and cb.tile(b) + b > 256 for b in range(1, 257))


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_coarse_kernel_metadata(device_asm):
    """k_coarse_sum<NV>, NV = 1 .. 8: no scratch in any instantiation and no static LDS, as include/bflbm.h states (the column
    sums are the launch's dynamic LDS, 2048 Q bytes).  One kernel per variable count is the whole sample: no second one."""
    found = kernels(device_asm, r"^_Z\w*?12k_coarse_sumILi(\d)EE\w*:")                  # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
        assert re.search(r"; LDSByteSize: 0\b", meta), f"{m.group(0)}: static LDS"
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_coarse_\w*:")) == 8


# ---- plotfiles --------------------------------------------------------------------------------------------------------------
def test_plotfiles_of_a_synthetic_record_read_back_bit_for_bit(pkg, tmp_path):
    """CoarseTrace.write_plotfiles on a record that never saw a device: one directory per sample under the step's name, the
    coarse cells as the box, the sums under their names; plotfile.read_plotfile returns the same bits."""
    rng = np.random.default_rng(11)
    sums = rng.standard_normal((3, 2, 4, 3, 2, 5))          # [count, B, Q, cz, cy, cx]
    sums[1, 1, 2, 0, 1, 3] = -0.0
    steps = np.array([[10, 1010], [20, 1020], [30, 1030]], dtype=np.int64)
    tr = object.__new__(pkg.CoarseTrace)                    # no owner, no handle: the record is given
    tr.source, tr.component_names = 0, pkg.plotfile.variable_names(22)
    tr.variables, tr.pairs = [0, 1, 2], [(0, 1)]
    tr.read = lambda first=0, count=None: (steps, sums)
    assert tr.sum_names == ["rho", "phi", "ufx", "rho*phi"]
    for replica in (0, 1):
        root = str(tmp_path / f"coarse_r{replica}_")
        names = tr.write_plotfiles(root, replica=replica)
        assert names == [pkg.plotfile.concatenate(root, int(s)) for s in steps[:, replica]]
        for k, name in enumerate(names):
            back, hdr = pkg.plotfile.read_plotfile(name)
            assert back.tobytes() == sums[k, replica].tobytes()
            assert hdr["names"] == tr.sum_names and hdr["n"] == (5, 2, 3) and hdr["step"] == steps[k, replica] and hdr["ncomp"] == 4
    with pytest.raises(ValueError):
        tr.write_plotfiles(str(tmp_path / "bad_"), replica=2)
