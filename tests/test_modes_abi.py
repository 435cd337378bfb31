"""Mode traces, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must fail before
any device is touched), the phase tables of bflbm_modes_phases, analysis.fourier_modes against numpy's fftn,
analysis.time_correlation on a planted series, the emulation of the kernels' order (tests/mode_sums.py) against an exact
reference inside its bound, and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import mode_sums as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES_SYMBOLS = ["bflbm_modes_create", "bflbm_batch_modes_create", "bflbm_modes_destroy", "bflbm_modes_sample",
                 "bflbm_modes_reset", "bflbm_modes_count", "bflbm_modes_geometry", "bflbm_modes_phases", "bflbm_modes_read"]
BOXES = [(13, 10, 6), (40, 9, 5)]


def test_modes_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in MODES_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert header.count("Mode traces:") == 1
    assert hasattr(pkg, "ModeTrace") and "ModeTrace" in pkg.__all__
    assert hasattr(pkg.BinaryLBM, "mode_trace") and hasattr(pkg.BatchLBM, "mode_trace")
    assert hasattr(pkg.analysis, "fourier_modes") and hasattr(pkg.analysis, "time_correlation")


def test_modes_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    g = [ctypes.c_int() for _ in range(4)]
    buf = (ctypes.c_double * 8)()
    va, mo = (ctypes.c_int * 1)(0), (ctypes.c_int * 3)(1, 0, 0)
    calls = {
        "bflbm_modes_create": lambda: lib.bflbm_modes_create(None, 1, va, 0, 1, mo, 1, 4, ctypes.byref(h)),
        "bflbm_batch_modes_create": lambda: lib.bflbm_batch_modes_create(None, 1, va, 0, 1, mo, 1, 4, ctypes.byref(h)),
        "bflbm_modes_sample": lambda: lib.bflbm_modes_sample(None),
        "bflbm_modes_reset": lambda: lib.bflbm_modes_reset(None),
        "bflbm_modes_count": lambda: lib.bflbm_modes_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_modes_geometry": lambda: lib.bflbm_modes_geometry(None, *[ctypes.byref(v) for v in g]),
        "bflbm_modes_phases": lambda: lib.bflbm_modes_phases(8, None),
        "bflbm_modes_read": lambda: lib.bflbm_modes_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_modes_destroy(None) == 0            # like every destroy of the ABI: nothing to do
    assert lib.bflbm_modes_phases(0, buf) != 0 and "bflbm_modes_phases" in lib.bflbm_last_error().decode()


# ---- the phase tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 12, 13, 16, 20, 40])
def test_phase_table(pkg, n):
    t = ms.phase_table(pkg._lib.load(), n)
    j = np.arange(n, dtype=np.longdouble)
    pi_l = np.arctan(np.longdouble(1)) * 4                # pi in longdouble, not the double rounded
    ang = 2 * pi_l * j / n
    want = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    err = np.abs(t.astype(np.longdouble) - want).max()
    print("n = %d: largest |T - longdouble| = %.3g (bound 2^-52 = %.3g)" % (n, float(err), 2.0 ** -52))
    assert err <= np.longdouble(2.0) ** -52
    for q in range(n):
        if 4 * q % n == 0:                                # the quarter points: exact, signed zeros allowed
            c, s = [(1, 0), (0, -1), (-1, 0), (0, 1)][4 * q // n]
            assert t[q, 0] == c and t[q, 1] == s, (n, q, t[q])
        if q:
            assert t[n - q, 0] == t[q, 0] and t[n - q, 1] == -t[q, 1], (n, q)
    assert t[0, 1] == 0


# ---- analysis.fourier_modes, analysis.time_correlation --------------------------------------------------------------------
@pytest.mark.parametrize("n", [(13, 10, 6), (40, 9, 5), (16, 12, 8), (7, 7, 7)])
def test_fourier_modes_equal_fftn(pkg, n):
    nx, ny, nz = n
    rng = np.random.default_rng(5)
    a = rng.standard_normal((2, nz, ny, nx))
    modes = np.concatenate([ms.issue_modes(n), [(-1, -1, -1), (nx // 2, 0, 0), (0, -(ny // 2), nz // 2), (nx + 2, -ny - 1, 3 * nz), (-nx, ny, 0)]])
    got = pkg.analysis.fourier_modes(a, modes)
    assert got.shape == (2, len(modes)) and got.dtype == np.complex128
    for r in range(2):
        hat = np.fft.fftn(a[r])
        want = np.array([hat[mz % nz, my % ny, mx % nx] for mx, my, mz in modes.tolist()])
        assert np.abs(got[r] - want).max() <= 1e-12 * np.abs(a[r]).sum()
    with pytest.raises(ValueError):
        pkg.analysis.fourier_modes(a, [(1.0, 0.0, 0.0)])
    with pytest.raises(ValueError):
        pkg.analysis.fourier_modes(a, [1, 0, 0])


def test_time_correlation_of_a_planted_series(pkg):
    z = 0.97 * np.exp(0.21j)
    t = np.arange(300)
    a = z ** t
    # a[t + lag] conj(a[t]) = z^lag |z|^(2t): the second series carries 1 / conj(z)^t, so that every product is z^lag
    b = 1.0 / np.conj(z) ** t
    c = pkg.analysis.time_correlation(a, b, max_lag=25)
    assert c.shape == (26,) and np.abs(c - z ** np.arange(26)).max() <= 1e-12
    # other axes pass through; b None is the auto-correlation; the default max_lag is every lag
    two = np.stack([a, 2 * a], axis=1)
    c2 = pkg.analysis.time_correlation(two, np.stack([b, b], axis=1), max_lag=5)
    assert c2.shape == (6, 2) and np.abs(c2[:, 1] - 2 * z ** np.arange(6)).max() <= 1e-12
    unit = np.exp(0.3j * t)
    auto = pkg.analysis.time_correlation(unit)
    assert auto.shape == (300,) and np.abs(auto - np.exp(0.3j * t)).max() <= 1e-12
    with pytest.raises(ValueError):
        pkg.analysis.time_correlation(a, b[:-1])
    with pytest.raises(ValueError):
        pkg.analysis.time_correlation(a, max_lag=300)


# ---- the order of the kernels' sums and its bound -------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES)
def test_emulated_order_is_inside_the_depth_bound(pkg, n):
    nx, ny, nz = n
    lib = pkg._lib.load()
    tables = ms.tables_of(lib, n)
    modes = ms.issue_modes(n)
    bound = ms.depth_bound(*n)
    d = 8 + ms.PER_THREAD + 8 + ms.tiles_per_plane(nx, ny) + nz
    assert bound == d * ms.U / (1 - d * ms.U)
    rng = np.random.default_rng(nx)
    for field in (0.5 + rng.random((nz, ny, nx)), rng.standard_normal((nz, ny, nx)) * 1e-3):
        got = ms.emulate(field, modes, tables)
        want = ms.exact(field, modes, tables)
        ratios = [ms.ratio_to_bound(g, w, np.abs(field).sum(), bound) for g, w in zip(got, want)]
        print(n, "|emulation - exact| / (depth_bound sum |a|) per wavevector:", ["%.3g" % r for r in ratios])
        assert max(ratios) <= 1.0
        # and the definition in numpy agrees with the exact sums over the library's tables to the tables' own error
        loose = pkg.analysis.fourier_modes(field, modes)
        assert max(ms.ratio_to_bound(g, w, np.abs(field).sum(), 1e-13) for g, w in zip(loose, want)) <= 1.0


def test_emulation_follows_the_tiles(pkg):
    """More than one tile per plane with a short last one: the emulation still sums every site once."""
    n = (70, 31, 3)                                       # 2170 sites per plane: tiles of 2048 and 122
    assert ms.tiles_per_plane(70, 31) == 2
    tables = ms.tables_of(pkg._lib.load(), n)
    field = np.random.default_rng(2).integers(1, 1000, size=n[::-1]).astype(np.float64)
    modes = np.array([(0, 0, 0), (35, 0, 0), (0, 0, 0)])
    got = ms.emulate(field, modes, tables)
    assert got[0] == field.sum() and got[1] == (field * (-1.0) ** np.arange(70)).sum() and got[2] == got[0]


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_modes_kernel_metadata(device_asm):
    """k_modes_project<NV>, NV = 1 .. 8, and k_modes_finish: no scratch, and the LDS size include/bflbm.h states."""
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    assert "36864 + 3072 nvars" in header and "61440" in header and "4096" in header
    found = kernels(device_asm, r"^_Z\w*?15k_modes_projectILi(\d)EE\w*:")     # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        nv = int(m.group(1))
        assert re.search(r"; ScratchSize: 0\b", meta), f"k_modes_project<{nv}> spills to scratch"
        assert re.search(r"; LDSByteSize: %d\b" % (36864 + 3072 * nv), meta), f"k_modes_project<{nv}>: not the LDS size include/bflbm.h states"
    finish = kernels(device_asm, r"^_Z\w*?14k_modes_finishE\w*:")
    assert len(finish) == 1
    assert re.search(r"; ScratchSize: 0\b", finish[0][1]) and re.search(r"; LDSByteSize: 4096\b", finish[0][1])
