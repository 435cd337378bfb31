"""Readers and comparisons for tests/golden/reference_*.npz (output of the reference's own compiled code, written by
tests/golden/make_golden_reference.py).  Shared by tests/test_reference_pins.py and tests/test_gpu_reference_pins.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_reference as mgr  # noqa: E402

FILES = ("trajectories", "tiling", "noise_injected", "noise_generated", "units")
_cache = {}

# Generated noise of modes 4..18 against the reference's field from the same normals, in ulp of the reference value.
# With K = 2 (l - l^2/2) kBT / cs2 b[a] (the same double on both sides: the same operations in the same order), r = |rho|,
# N the normal and u = 2^-53, every operation rounding once with relative error <= u:
#   reference (LBM_binary.H:125-126)  fl(fl(sqrt(fl(K r))) N):  sqrt halves the error of its argument: u/2, + u for the
#                                     square root, + u for the product                                   -> <= 2.5 u
#   project                           fl(fl(fl(sqrt K) fl(sqrt r)) N): two square roots, two products     -> <= 4 u
# so the two differ by at most 6.5 u (1 + O(u)) relative to the exact value, and one ulp of a double v is > u |v|:
# at most 6.5 ulp (a multiple of 1/2 only when the two fall into different binades).  Modes 1..3 (:117) are evaluated
# literally and must be equal.
NOISE_ULP_BOUND = 6.5


def fixture(name):
    if name not in _cache:
        _cache[name] = mgr.load(name)
    return _cache[name]


def cases(name):
    return fixture(name)[0]["cases"]


def same(a, b):
    """Equal as numbers: -0.0 == +0.0 (fixtures hash x + 0.0), NaN equals NaN."""
    a, b = np.asarray(a) + 0.0, np.asarray(b) + 0.0
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def mismatch(got, want):
    """'' when `got` equals the stored entry (an array, or a SHA-256 digest of x + 0.0), else a description."""
    if want.dtype == np.uint8:
        return "" if np.array_equal(mgr.digest(got), want) else "digest differs"
    got = got[:want.shape[0]]
    if same(got, want):
        return ""
    with np.errstate(all="ignore"):
        d = np.abs(got - want)
    return f"{np.count_nonzero(~((got + 0.0 == want + 0.0) | (np.isnan(got) & np.isnan(want))))} of {want.size} differ, max |d| = {np.nanmax(d):.3e}"


def assert_record(z, key, got, what=""):
    """got: {"f","g","hbar","h"} arrays against z[key/<name>]: an array (of the leading components where the fixture
    keeps fewer) or a digest, and the digest z[key/<name>_digest] of the whole array where the fixture has both."""
    bad = []
    for nm, arr in got.items():
        for k in (f"{key}/{nm}", f"{key}/{nm}_digest"):
            if k in z and mismatch(arr, z[k]):
                bad.append(f"{k}: {mismatch(arr, z[k])}")
        assert f"{key}/{nm}" in z, f"{key}/{nm} is not in the fixture"
    assert not bad, f"{what} differs from the reference: " + "; ".join(bad)


def ulp_distance(got, ref):
    """Largest |got - ref| in units of the spacing of the doubles at |ref|; inf where `got` is not finite."""
    got, ref = np.asarray(got), np.asarray(ref)
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    m = d > 0
    return float((d[m] / np.spacing(np.abs(ref[m]))).max()) if m.any() else 0.0


def assert_noise(fn, gn, ref_fn, ref_gn, what):
    """Modes 0..3 equal, modes 4..18 within NOISE_ULP_BOUND; -> the measured maximum in ulp."""
    assert same(fn[:4], ref_fn[:4]) and same(gn[:4], ref_gn[:4]), f"{what}: modes 0..3 differ from the reference"
    worst = max(ulp_distance(fn[4:], ref_fn[4:]), ulp_distance(gn[4:], ref_gn[4:]))
    print(f"[noise ulp] {what}: max {worst:g} ulp (bound {NOISE_ULP_BOUND})")
    assert worst <= NOISE_ULP_BOUND, f"{what}: generated noise {worst:g} ulp from the reference's field (bound {NOISE_ULP_BOUND})"
    return worst


def initial_state(z, name, case):
    """(f0, g0) of an uploaded case, else None (the case starts from one of the three analytic inits)."""
    return (z[f"{name}/f0"], z[f"{name}/g0"]) if case["init"][0] == "upload" else None
