"""Histogram traces, CPU side: analysis.field_histograms against a site-by-site loop of the binning rule in Python
floats (tests/hist_counts.py), the block sums, analysis.histogram_moments against its derived bound, the C-ABI surface
(declared, exported, bound with the header's argument lists), the null-pointer refusals (which must fail before any
device is touched), the host part of csrc/bflbm_hist.h through a stand-alone program built with the address and
undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import hist_counts as hc
import profile_sums as ps
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

HIST_SYMBOLS = ["bflbm_hist_create", "bflbm_batch_hist_create", "bflbm_ring_hist_create", "bflbm_hist_destroy", "bflbm_hist_sample",
                "bflbm_hist_reset", "bflbm_hist_count", "bflbm_hist_geometry", "bflbm_hist_read"]
LO, HI, NBINS = [0.0, -1.5, 1e-3], [1.0, 2.5, 1.25e-3], [7, 16, 5]
PAIRS = [(0, 1), (2, 0)]


def _fields(n, seed=None):
    """Three fields of a box that straddle their ranges, with the planted values of every variable at chosen sites."""
    nx, ny, nz = n
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz if seed is None else seed)
    x = np.empty((3, nz, ny, nx))
    for v in range(3):
        w = HI[v] - LO[v]
        x[v] = rng.uniform(LO[v] - 0.2 * w, HI[v] + 0.2 * w, size=(nz, ny, nx))
        flat = x[v].reshape(-1)
        plant = hc.planted(LO[v], HI[v])
        at = rng.choice(flat.size, size=len(plant), replace=False)
        flat[at] = plant
    return x


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.BOXES)
def test_field_histograms_against_the_brute_force_loop(pkg, n):
    """Integer for integer, with lo, hi, nextafter(hi, -inf), -0.0, +inf, -inf and NaN planted in every variable; every
    variable block and every pair block sums to the site count."""
    x = _fields(n)
    got = pkg.analysis.field_histograms(x, LO, HI, NBINS, PAIRS)
    want = hc.brute(x, LO, HI, NBINS, PAIRS)
    C, blk = hc.blocks(NBINS, PAIRS)
    assert got.dtype == np.int64 and got.shape == (C,) and np.array_equal(got, want), n
    assert pkg.analysis.histogram_blocks(NBINS, PAIRS) == (C, blk)
    assert hc.block_sums(got, blk).tolist() == [n[0] * n[1] * n[2]] * 5
    for v in range(3):                                     # the planted values went where the rule sends them
        off, length = blk[v]
        below, above, nan = got[off + length - 3:off + length]
        assert nan >= 1 and below >= 1 and above >= 2


def test_planted_values_land_where_the_rule_says(pkg):
    """One variable, the planted values alone.  [0, 1) in 10 bins: lo and -0.0 in bin 0, hi and +inf above, -inf below,
    NaN in nan, nextafter(1, -inf) * 10 = 9.999999999999998 in bin 9.  [-0.5, 1.8) in 13 bins: the scale 13 / 2.3 is
    rounded up and (nextafter(1.8, -inf) + 0.5) * scale rounds to 13.0: above, by the rule; -0.0 is 0.5 * scale = 2.8...:
    bin 2."""
    plant = np.array([hc.planted(0.0, 1.0)])
    got = pkg.analysis.field_histograms(plant, [0.0], [1.0], [10])
    assert got.tolist() == [2] + [0] * 8 + [1] + [1, 2, 1], got
    plant13 = np.array([hc.planted(-0.5, 1.8)])
    got13 = pkg.analysis.field_histograms(plant13, [-0.5], [1.8], [13])
    assert got13.tolist() == [1, 0, 1] + [0] * 10 + [1, 3, 1], got13
    assert np.array_equal(got, hc.brute(plant, [0.0], [1.0], [10])) and np.array_equal(got13, hc.brute(plant13, [-0.5], [1.8], [13]))


def test_field_histograms_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((2, 3, 4, 5))
    for bad in (lambda: an.field_histograms(f, [0, 0], [1, 1], [4]), lambda: an.field_histograms(f, [0, 1], [1, 1], [4, 4]),
                lambda: an.field_histograms(f, [0, np.nan], [1, 1], [4, 4]), lambda: an.field_histograms(f, [0, 0], [1, np.inf], [4, 4]),
                lambda: an.field_histograms(f, [0, 0], [1, 1], [4, 0]), lambda: an.field_histograms(f, [0, 0], [1, 1], [4, 4097]),
                lambda: an.field_histograms(f, [0, 0], [1, 1], [4, 4], [(0, 0)]), lambda: an.field_histograms(f, [0, 0], [1, 1], [4, 4], [(0, 2)]),
                lambda: an.field_histograms(f, [0, 0], [1, 1], [4, 4], [(0, 1)] * 5),
                lambda: an.field_histograms(f, [0, 0], [1, 1], [127, 127], [(0, 1)]),
                lambda: an.field_histograms(f, [-1.7e308, 0], [1.7e308, 1], [4, 4]), lambda: an.field_histograms(f, [0, 0], [5e-324, 1], [4, 4])):
        with pytest.raises(ValueError):
            bad()
    assert an.field_histograms(f, [0, 0], [1, 1], [127, 126], [(0, 1)]).shape == (16262,)


@pytest.mark.parametrize("n", [(7, 9, 5), (64, 32, 3)])
def test_histogram_moments_lie_within_half_a_bin_width(pkg, n):
    """Every in-range value lies within w / 2 of the centre of its bin, so the histogram mean lies within w / 2 of the
    in-range mean: derived, not measured.  (The rounding of t and of the two means is some 1e-16 of the range.)"""
    x = _fields(n)
    C, blk = hc.blocks(NBINS, PAIRS)
    counts = pkg.analysis.field_histograms(x, LO, HI, NBINS, PAIRS)
    for v in range(3):
        off, length = blk[v]
        flat = x[v].reshape(-1)
        with np.errstate(invalid="ignore"):
            t = (flat - LO[v]) * (NBINS[v] / (HI[v] - LO[v]))
            inside = flat[(t >= 0) & (t < NBINS[v])]
        mean, var = pkg.analysis.histogram_moments(counts[off:off + length - 3], LO[v], HI[v])
        w = (HI[v] - LO[v]) / NBINS[v]
        print(n, v, "|histogram mean - in-range mean| / w = %.4f, histogram variance / in-range variance = %.4f"
              % (abs(mean - inside.mean()) / w, var / inside.var()))
        assert counts[off:off + length - 3].sum() == inside.size
        assert abs(mean - inside.mean()) <= 0.5 * w and var >= 0
    m, s = pkg.analysis.histogram_moments(np.zeros((2, 4)), 0.0, 1.0)       # no site in range
    assert m.shape == (2,) and np.isnan(m).all() and np.isnan(s).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_hist_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in HIST_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_hist_create"] == sig["bflbm_batch_hist_create"] == sig["bflbm_ring_hist_create"]
    # (owner, source, nvars, vars, lo, hi, nbins, npairs, pair_a, pair_b, every, capacity, out)
    assert len(sig["bflbm_hist_create"][1]) == 13 and sig["bflbm_hist_create"][1][11] is ctypes.c_longlong
    assert sig["bflbm_hist_read"][1][3] == ctypes.POINTER(ctypes.c_longlong)          # integers, not doubles
    assert header.count("Histogram traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert hasattr(pkg, "HistogramTrace") and "HistogramTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM, pkg.RingLBM):
        assert hasattr(owner, "histogram_trace")
    for fn in ("field_histograms", "histogram_moments", "histogram_blocks"):
        assert hasattr(pkg.analysis, fn)
    # the header, the numpy twin and the tests' helper state the same constants
    an = pkg.analysis
    assert (an.HIST_MAX_BINS, an.HIST_MAX_PAIRS, an.HIST_MAX_COUNTERS) == (4096, 4, hc.MAX_COUNTERS)
    block = header[header.index("Histogram traces:"):header.index("typedef struct bflbm_hist")]
    for words in ("nbins_v in 1..4096", "npairs in 0..4", "C <= 16384", "tiles of 2048 consecutive sites", "16384 bytes for C <= 4096",
                  "else 65536 bytes", "max(1, 512 / replicas)", "2^31 sites"):
        assert words in block, words


def test_hist_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_longlong * 8)()
    va, nb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(4)
    lo, hi = (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(1.0)
    g = [ctypes.c_int() for _ in range(7)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 1, va, lo, hi, nb, 0, None, None, 1, 4, ctypes.byref(h)))
             for name in HIST_SYMBOLS[:3]}
    calls.update({
        "bflbm_hist_sample": lambda: lib.bflbm_hist_sample(None),
        "bflbm_hist_reset": lambda: lib.bflbm_hist_reset(None),
        "bflbm_hist_count": lambda: lib.bflbm_hist_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_hist_geometry": lambda: lib.bflbm_hist_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_hist_read": lambda: lib.bflbm_hist_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_hist_destroy(None) == 0                # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_layout_and_refusals_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "hist_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "hist_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 46  # the checks hist_main.cpp makes: a check that silently stops running fails here


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_hist_kernel_metadata(device_asm):
    """k_hist_count<NV, CCAP>, NV = 1 .. 8, CCAP = 4096 and 16384, and k_hist_finish: no scratch; the counting kernel's LDS
    is the 4 CCAP bytes include/bflbm.h states (16384 bytes for C <= 4096, else 65536), the finishing kernel uses none."""
    found = kernels(device_asm, r"^_Z\w*?12k_hist_countILi(\d)ELi(\d+)EE\w*:")      # Itanium mangling: <length><name>
    assert sorted((int(m.group(1)), int(m.group(2))) for m, _ in found) == [(nv, c) for nv in range(1, 9) for c in (4096, 16384)]
    for m, meta in found:
        assert int(m.group(2)) == hc.lds_counters(int(m.group(2)))
        assert re.search(r"; LDSByteSize: %d\b" % (4 * int(m.group(2))), meta), f"{m.group(0)}: LDS"
    finish = kernels(device_asm, r"^_Z\w*?13k_hist_finish(E)\w*:")
    assert len(finish) == 1 and re.search(r"; LDSByteSize: 0\b", finish[0][1])
    for m, meta in found + finish:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
