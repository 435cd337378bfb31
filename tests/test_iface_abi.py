"""Interface traces, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must fail
before any device is touched), analysis.interface_heights and analysis.capillary_spectrum against plain loops, and the
compiled kernels (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernel_of, mangled   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IFACE_SYMBOLS = ["bflbm_iface_create", "bflbm_batch_iface_create", "bflbm_iface_destroy", "bflbm_iface_sample",
                 "bflbm_iface_reset", "bflbm_iface_count", "bflbm_iface_geometry", "bflbm_iface_read"]


def test_iface_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in IFACE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert hasattr(pkg, "InterfaceTrace") and "InterfaceTrace" in pkg.__all__
    assert hasattr(pkg.BinaryLBM, "interface_trace") and hasattr(pkg.BatchLBM, "interface_trace")


def test_iface_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    g = [ctypes.c_int() for _ in range(4)]
    buf = (ctypes.c_double * 8)()
    calls = {
        "bflbm_iface_create": lambda: lib.bflbm_iface_create(None, 0, 0.5, 0, 8, 1, 4, ctypes.byref(h)),
        "bflbm_batch_iface_create": lambda: lib.bflbm_batch_iface_create(None, 0, 0.5, 0, 8, 1, 4, ctypes.byref(h)),
        "bflbm_iface_sample": lambda: lib.bflbm_iface_sample(None),
        "bflbm_iface_reset": lambda: lib.bflbm_iface_reset(None),
        "bflbm_iface_count": lambda: lib.bflbm_iface_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_iface_geometry": lambda: lib.bflbm_iface_geometry(None, *[ctypes.byref(v) for v in g]),
        "bflbm_iface_read": lambda: lib.bflbm_iface_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name.split(" ")[0] in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_iface_destroy(None) == 0            # like every destroy of the ABI: nothing to do


# ---- analysis.interface_heights against a plain triple loop ----------------------------------------------------------
def _heights_loop(d, level, z_lo, z_hi):
    """The definition of include/bflbm.h, one column and one pair at a time, in Python floats (IEEE doubles)."""
    nz, ny, nx = d.shape
    out = np.full((2, ny, nx), np.nan)
    for y in range(ny):
        for x in range(nx):
            seen = [False, False]
            for z in range(z_lo + 1, z_hi):
                a, b = float(d[z - 1, y, x]), float(d[z, y, x])
                hit = (a < level <= b, a >= level > b)
                for k in range(2):
                    if hit[k] and not seen[k]:
                        out[k, y, x] = float(z - 1) + (level - a) / (b - a)
                        seen[k] = True
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_interface_heights_against_a_triple_loop(pkg):
    rng = np.random.default_rng(5)
    nz, ny, nx = 13, 5, 7
    level = 0.5
    d = 0.5 + 0.3 * rng.standard_normal((nz, ny, nx))                 # many crossings per column, both ways
    d[:, 0, 0] = 0.1                                                     # a column that never reaches the level
    d[:, 1, 2] = np.linspace(0.0, 1.0, nz)                               # one planted rising crossing, no falling one
    d[:, 2, 3] = np.linspace(1.0, 0.0, nz)                               # one planted falling crossing, no rising one
    for window in (None, (0, nz), (3, 9), (4, 6), (11, 13)):
        z_lo, z_hi = (0, nz) if window is None else window
        got = pkg.analysis.interface_heights(d, level, window)
        want = _heights_loop(d, level, z_lo, z_hi)
        assert got.shape == (2, ny, nx) and _same(got, want), window
    full = pkg.analysis.interface_heights(d, level)
    assert np.isnan(full[:, 0, 0]).all()
    assert not np.isnan(full[0, 1, 2]) and np.isnan(full[1, 1, 2])
    assert np.isnan(full[0, 2, 3]) and not np.isnan(full[1, 2, 3])
    assert 0 < np.isnan(full).sum() < full.size
    for bad in ((-1, 5), (0, nz + 1), (4, 5)):
        with pytest.raises(ValueError):
            pkg.analysis.interface_heights(d, level, bad)


def test_interface_heights_edge_cases(pkg):
    level = 0.5
    # a value exactly equal to the level: as d(z) it closes a rising pair, as d(z-1) it opens a falling pair
    col = np.array([0.2, 0.5, 0.9, 0.5, 0.1, 0.5, 0.5, 0.7])
    d = col[:, None, None].repeat(2, axis=2)
    got = pkg.analysis.interface_heights(d, level)
    assert _same(got, _heights_loop(d, level, 0, len(col)))
    assert got[0, 0, 0] == 1.0                           # rising at the pair (0, 1): 0 + (0.5 - 0.2) / (0.5 - 0.2)
    assert got[1, 0, 0] == 3.0                           # falling at the pair (3, 4): d(3) == level counts as "at or above"
    assert np.array_equal(pkg.analysis.interface_heights(d, level, (4, 8))[:, 0, 0], [5.0, np.nan], equal_nan=True)   # 4 + (0.5 - 0.1) / (0.5 - 0.1)
    # a pair with both values at the level is no crossing either way
    flat = np.full((4, 1, 1), level)
    assert np.isnan(pkg.analysis.interface_heights(flat, level)).all()
    # no crossing at all
    assert np.isnan(pkg.analysis.interface_heights(d, 2.0)).all()
    assert np.isnan(pkg.analysis.interface_heights(d, -1.0)).all()
    # a NaN site satisfies neither condition: the crossing through it is lost, the next one is found
    e = np.array([0.2, np.nan, 0.9, 0.1, 0.8])[:, None, None]
    got = pkg.analysis.interface_heights(e, level)
    assert _same(got, _heights_loop(e, level, 0, 5))
    assert got[1, 0, 0] == 2.0 + (0.5 - 0.9) / (0.1 - 0.9) and got[0, 0, 0] == 3.0 + (0.5 - 0.1) / (0.8 - 0.1)
    assert np.isnan(pkg.analysis.interface_heights(np.full((3, 1, 1), np.nan), level)).all()


# ---- analysis.capillary_spectrum against a direct DFT sum ---------------------------------------------------------------
def test_capillary_spectrum_against_a_direct_sum(pkg):
    """Bound: the direct sum and the FFT add the same n terms h_j exp(-i q j) in another order, so each is within
    n eps sum|h_j| of the exact sum and the two within err = 2 n eps sum|h_j| of each other (the a-priori bound of a
    re-ordered sum, as in tests/test_gpu_trace.py).  |h_q|^2 then differs by at most 2 |h_q| err + err^2; the mean over
    T keeps the largest such bound, and the squares and the mean themselves round a few eps relative."""
    rng = np.random.default_rng(3)
    eps = 2.0 ** -53
    T, ny, nx = 6, 5, 12
    h = 24.0 + 0.05 * rng.standard_normal((T, ny, nx))

    # one axis (the notebook's cell 9 on every line)
    got, (q,) = pkg.analysis.capillary_spectrum(h)
    assert got.shape == (ny, nx) and np.array_equal(q, 2 * np.pi * np.fft.fftfreq(nx))
    dev = h - h.mean(axis=0)
    for y in range(ny):
        for m in range(nx):
            acc, worst = 0.0, 0.0
            for t in range(T):
                s = sum(dev[t, y, j] * complex(math.cos(2 * math.pi * m * j / nx), -math.sin(2 * math.pi * m * j / nx)) for j in range(nx))
                err = 2 * nx * eps * np.abs(dev[t, y]).sum()
                acc += abs(s) ** 2
                worst = max(worst, 2 * abs(s) * err + err * err)
            bound = worst + 4 * eps * acc / T              # the squares and the mean themselves
            assert abs(got[y, m] - acc / T) <= bound, (y, m, got[y, m], acc / T, bound)

    # both in-plane axes
    got2, (qy, qx) = pkg.analysis.capillary_spectrum(h, axes=(-2, -1))
    assert got2.shape == (ny, nx)
    assert np.array_equal(qy, 2 * np.pi * np.fft.fftfreq(ny)) and np.array_equal(qx, 2 * np.pi * np.fft.fftfreq(nx))
    n = ny * nx
    for my in range(ny):
        for mx in range(nx):
            acc, worst = 0.0, 0.0
            for t in range(T):
                s = 0j
                for jy in range(ny):
                    for jx in range(nx):
                        ang = 2 * math.pi * (my * jy / ny + mx * jx / nx)
                        s += dev[t, jy, jx] * complex(math.cos(ang), -math.sin(ang))
                err = 2 * n * eps * np.abs(dev[t]).sum()
                acc += abs(s) ** 2
                worst = max(worst, 2 * abs(s) * err + err * err)
            bound = worst + 4 * eps * acc / T
            assert abs(got2[my, mx] - acc / T) <= bound, (my, mx)
    with pytest.raises(ValueError):
        pkg.analysis.capillary_spectrum(h, axes=(0,))      # axis 0 is time
    with pytest.raises(ValueError):
        pkg.analysis.capillary_spectrum(h[0, 0])


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k_iface_scan", "k_iface_scan_batch", "k_iface_finish"])
def test_iface_kernel_compiled_without_scratch(device_asm, kernel):
    _, meta = kernel_of(device_asm, mangled(kernel), "interface kernel")
    assert re.search(r"; ScratchSize: 0\b", meta), f"{kernel} spills to scratch"
