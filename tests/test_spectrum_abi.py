"""Spectrum traces, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must fail
before any device is touched), analysis.spectrum_bins against the mode counts the definition lists and against a plain
loop, analysis.binned_spectrum against Parseval's sum, analysis.domain_length of a single mode, and the compiled
kernels (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernel_of, mangled   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECTRUM_SYMBOLS = ["bflbm_spectrum_create", "bflbm_batch_spectrum_create", "bflbm_spectrum_destroy", "bflbm_spectrum_sample",
                    "bflbm_spectrum_reset", "bflbm_spectrum_count", "bflbm_spectrum_geometry", "bflbm_spectrum_bins",
                    "bflbm_spectrum_read"]
SHAPES = [(16, 16, 16), (12, 10, 14), (9, 7, 5), (8, 32, 16), (32, 32, 32)]
KINDS = ["shell", "x", "y", "z"]


def test_spectrum_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in SPECTRUM_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert "Spectrum traces" in header
    assert hasattr(pkg, "SpectrumTrace") and "SpectrumTrace" in pkg.__all__
    assert hasattr(pkg.BinaryLBM, "spectrum_trace") and hasattr(pkg.BatchLBM, "spectrum_trace")


def test_spectrum_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    g = [ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()]
    buf = (ctypes.c_double * 8)()
    cnt = (ctypes.c_longlong * 8)()
    va, vb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    calls = {
        "bflbm_spectrum_create": lambda: lib.bflbm_spectrum_create(None, 1, va, vb, None, 0, 0, 1, 1, 4, ctypes.byref(h)),
        "bflbm_batch_spectrum_create": lambda: lib.bflbm_batch_spectrum_create(None, 1, va, vb, None, 0, 0, 1, 1, 4, ctypes.byref(h)),
        "bflbm_spectrum_sample": lambda: lib.bflbm_spectrum_sample(None),
        "bflbm_spectrum_reset": lambda: lib.bflbm_spectrum_reset(None),
        "bflbm_spectrum_count": lambda: lib.bflbm_spectrum_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_spectrum_geometry": lambda: lib.bflbm_spectrum_geometry(None, *[ctypes.byref(v) for v in g]),
        "bflbm_spectrum_bins": lambda: lib.bflbm_spectrum_bins(None, cnt, buf),
        "bflbm_spectrum_read": lambda: lib.bflbm_spectrum_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_spectrum_destroy(None) == 0         # like every destroy of the ABI: nothing to do


# ---- analysis.spectrum_bins ---------------------------------------------------------------------------------------------
# the mode counts stated with the definition (include/bflbm.h, "Spectrum traces"; found with a numpy prototype of it)
LISTED = [((16, 16, 16), "shell", 15, [1, 18, 62, 98, 210, 350]),
          ((8, 32, 16), "shell", 29, [1, 2, 8, 6, 34, 38]),
          ((9, 7, 5), "shell", 8, [1, 4, 28, 44, 94, 92]),
          ((12, 10, 14), "x", 7, [140, 280, 280]),
          ((12, 10, 14), "y", 6, [168, 336, 336, 336, 336, 168])]


@pytest.mark.parametrize("n,kind,nbins,head", LISTED)
def test_spectrum_bins_reproduces_the_listed_counts(pkg, n, kind, nbins, head):
    bins, count, q = pkg.analysis.spectrum_bins(n, kind, zero_avg=False)
    assert bins.shape == n[::-1] and len(count) == len(q) == nbins
    assert count[:len(head)].tolist() == head
    assert count.sum() == n[0] * n[1] * n[2] and bins.min() == 0
    bz, cz, qz = pkg.analysis.spectrum_bins(n, kind, zero_avg=True)
    assert cz.sum() == n[0] * n[1] * n[2] - 1 and cz[0] == count[0] - 1 and np.array_equal(cz[1:], count[1:])
    assert bz[0, 0, 0] == -1 and np.array_equal(bz.ravel()[1:], bins.ravel()[1:])
    assert np.array_equal(np.bincount(bz[bz >= 0], minlength=nbins), cz)


def _bins_loop(n, kind):
    """The definition one mode at a time, in Python integers and floats."""
    nx, ny, nz = n
    L = math.lcm(nx, ny, nz)
    W = L // max(n)
    out = np.empty((nz, ny, nx), dtype=np.int64)
    qs = {}
    for mz in range(nz):
        for my in range(ny):
            for mx in range(nx):
                k = [m if 2 * m <= s else m - s for m, s in zip((mx, my, mz), n)]       # signed, in (-n/2, n/2]
                if kind == 0:
                    K2 = sum((abs(ki) * (L // s)) ** 2 for ki, s in zip(k, n))
                    s_ = 0
                    while not ((s_ == 0 or (2 * s_ - 1) ** 2 * W * W <= 4 * K2) and 4 * K2 < (2 * s_ + 1) ** 2 * W * W):
                        s_ += 1
                else:
                    s_ = abs(k[kind - 1])
                out[mz, my, mx] = s_
                qs.setdefault(s_, []).append(2 * math.pi * math.sqrt(sum((ki / s) ** 2 for ki, s in zip(k, n))))
    return out, qs


@pytest.mark.parametrize("n", [(9, 7, 5), (8, 32, 16), (12, 10, 14), (6, 6, 6)])
def test_spectrum_bins_against_a_plain_loop(pkg, n):
    for kind in range(4):
        want, qs = _bins_loop(n, kind)
        bins, count, q = pkg.analysis.spectrum_bins(n, kind, zero_avg=False)
        assert np.array_equal(bins, want), (n, kind)
        for s in range(len(count)):
            assert count[s] == len(qs.get(s, []))
            if kind == 0 and count[s]:
                assert abs(q[s] - math.fsum(qs[s]) / count[s]) <= 1e-14 * q[s]
            elif kind == 0:
                assert np.isnan(q[s])
            else:
                assert q[s] == 2.0 * np.pi * s / n[kind - 1]
    # a cubic box: the usual round(|k|) shells
    if n[0] == n[1] == n[2]:
        k = np.fft.fftfreq(n[0], 1.0 / n[0])
        r = np.sqrt(k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, :] ** 2)
        assert np.array_equal(pkg.analysis.spectrum_bins(n, 0, zero_avg=False)[0], np.floor(r + 0.5).astype(np.int64))


def test_spectrum_bins_refusals(pkg):
    with pytest.raises(ValueError):
        pkg.analysis.spectrum_bins((8, 8, 8), 4)
    with pytest.raises(ValueError):
        pkg.analysis.spectrum_bins((8, 8, 8), "w")
    with pytest.raises(ValueError, match="63 bits"):
        pkg.analysis.spectrum_bins((65521, 65519, 65497), "shell")      # three primes: lcm ~ 2.8e14


# ---- analysis.binned_spectrum: Parseval ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_binned_spectrum_sums_to_the_real_space_product(pkg, n):
    """sum_k a^(k) conj(b^(k)) / N = sum_x a(x) b(x) (Parseval, unnormalised DFT); the bins partition the full spectrum."""
    rng = np.random.default_rng(11)
    a = rng.standard_normal(n[::-1])
    b = rng.standard_normal(n[::-1]) + 0.5 * a
    for kind in KINDS:
        for pair in ((a, a), (a, b)):
            s = pkg.analysis.binned_spectrum(pair[0], pair[1], kind, zero_avg=False)
            want = float((pair[0] * pair[1]).sum())
            assert abs(s.sum() - want) <= 1e-13 * abs(want), (n, kind)
            z = pkg.analysis.binned_spectrum(pair[0], pair[1], kind, zero_avg=True)
            assert np.array_equal(z[1:], s[1:])
            assert abs((s[0] - z[0]) - pair[0].sum() * pair[1].sum() / a.size) <= 1e-13 * abs(want)      # the k = 0 mode
        plain = pkg.analysis.binned_spectrum(a, b, kind)
        assert np.abs(pkg.analysis.binned_spectrum(a, b, kind, scale=3.0) - 3.0 * plain).max() <= 1e-13 * np.abs(plain).max()
    with pytest.raises(ValueError):
        pkg.analysis.binned_spectrum(a, b[:-1], "shell")


# ---- analysis.domain_length ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(24, 8, 6), (16, 16, 16)])
def test_domain_length_of_a_single_mode(pkg, n):
    nx, ny, nz = n
    x = np.arange(nx)
    a = np.broadcast_to(np.cos(2 * np.pi * 3 * x / nx), (nz, ny, nx)).copy()
    _, count, q = pkg.analysis.spectrum_bins(n, "x")
    s = pkg.analysis.binned_spectrum(a, a, "x")
    assert s[3] > 0.49 * a.size and np.abs(np.delete(s, 3)).max() <= 1e-12 * s[3]       # the power sits in |kx| = 3
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, s / count, np.nan)
    L = pkg.analysis.domain_length(q, mean)
    assert abs(L - nx / 3) <= 1e-11 * nx / 3
    both = pkg.analysis.domain_length(q, np.stack([mean, 2 * mean]))                      # leading axes pass through
    assert both.shape == (2,) and np.allclose(both, nx / 3, rtol=1e-11, atol=0)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,lds", [("k_spectrum_bin", 2048), ("k_spectrum_finish", 0)])
def test_spectrum_kernel_compiled_without_scratch_or_atomics(device_asm, kernel, lds):
    body, meta = kernel_of(device_asm, mangled(kernel), "spectrum kernel")
    assert not [l for l in body if "atomic" in l], f"{kernel} uses atomics"
    assert re.search(r"; ScratchSize: 0\b", meta), f"{kernel} spills to scratch"
    assert re.search(r"; LDSByteSize: %d\b" % lds, meta), f"{kernel}: LDS beyond the tree of 256 doubles"
