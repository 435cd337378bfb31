"""Field statistics, CPU side: analysis.field_statistics against a plain two-pass numpy mean and covariance, the C-ABI
surface (declared, exported, bound with the header's argument lists), the null-pointer refusals (which must fail before
any device is touched) and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FSTAT_SYMBOLS = ["bflbm_fstat_create", "bflbm_batch_fstat_create", "bflbm_ring_fstat_create", "bflbm_fstat_destroy",
                 "bflbm_fstat_sample", "bflbm_fstat_reset", "bflbm_fstat_count", "bflbm_fstat_get"]


# ---- the numpy restatement -------------------------------------------------------------------------------------------------
def test_field_statistics_against_two_pass_numpy(pkg):
    """40 frames of [3][4][5][6], O(1) values plus 1e-3 noise.  mean is exactly the sequential sum times 1.0 / N; cov is
    within 64 eps N max|x - first|^2 of the two-pass covariance: N rounded products of that size and their N additions."""
    rng = np.random.default_rng(11)
    n = 40
    base = 0.5 + rng.random((3, 4, 5, 6))
    frames = base[None] + 1e-3 * rng.standard_normal((n, 3, 4, 5, 6))
    pairs = [(0, 0), (0, 1), (2, 1), (2, 2)]
    st = pkg.analysis.field_statistics(frames, pairs)
    assert st["N"] == n and st["sum"].shape == (3, 4, 5, 6) and st["prod"].shape == (4, 4, 5, 6)
    seq = frames[0].copy()
    for t in range(1, n):
        seq = seq + frames[t]
    assert np.array_equal(st["first"], frames[0]) and np.array_equal(st["sum"], seq)
    assert np.array_equal(st["mean"], seq * (1.0 / n))
    two_pass_mean = frames.mean(axis=0)
    bound = 64 * np.finfo(np.float64).eps * n * np.abs(frames - frames[0]).max() ** 2
    for p, (a, b) in enumerate(pairs):
        want = ((frames[:, a] - two_pass_mean[a]) * (frames[:, b] - two_pass_mean[b])).mean(axis=0)
        err = np.abs(st["cov"][p] - want).max()
        print("pair", (a, b), "largest |cov - two pass| = %.3g, bound %.3g, largest |cov| = %.3g" % (err, bound, np.abs(want).max()))
        assert err <= bound
    # frame 0 alone: no spread, and +0.0 in prod
    one = pkg.analysis.field_statistics(frames[:1], pairs)
    assert not one["prod"].any() and not np.signbit(one["prod"]).any() and not one["cov"].any()
    assert np.array_equal(one["mean"], frames[0])
    with pytest.raises(ValueError):
        pkg.analysis.field_statistics(frames, [(0, 3)])
    with pytest.raises(ValueError):
        pkg.analysis.field_statistics(frames[:0], [])


def test_field_statistics_ensemble(pkg):
    rng = np.random.default_rng(12)
    frames = 1.0 + 1e-3 * rng.standard_normal((3, 7, 2, 2, 3, 4))         # [B][N][nvars][nz][ny][nx]
    reps = [pkg.analysis.field_statistics(f, [(0, 1), (1, 1)]) for f in frames]
    ens = pkg.analysis.field_statistics_ensemble(reps)
    total = ((0.0 + reps[0]["sum"]) + reps[1]["sum"]) + reps[2]["sum"]
    cov = ((0.0 + reps[0]["cov"]) + reps[1]["cov"]) + reps[2]["cov"]
    assert np.array_equal(ens["mean"], total * (1.0 / (3.0 * 7.0))) and np.array_equal(ens["cov"], cov * (1.0 / 3.0))
    assert np.abs(ens["mean"] - frames.mean(axis=(0, 1))).max() < 1e-15
    with pytest.raises(ValueError):
        pkg.analysis.field_statistics_ensemble([reps[0], pkg.analysis.field_statistics(frames[1][:3], [(0, 1), (1, 1)])])


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
_C_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}


def _declared_arguments(header, name):
    """The ctypes argument list the declaration of `name` in include/bflbm.h asks for: handles and output buffers are
    void pointers, as everywhere in _lib.SIGNATURES."""
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, f"{name} not declared in include/bflbm.h"
    out = []
    for arg in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        words = arg.replace("*", " * ").split()
        stars = words.count("*")
        base = " ".join(w for w in words[:-1] if w not in ("const", "*"))
        if stars == 0:
            out.append(_C_TYPES[base])
        elif stars == 1 and base in ("int", "long long"):
            out.append(ctypes.POINTER(_C_TYPES[base]))
        elif stars == 2:
            out.append(ctypes.POINTER(ctypes.c_void_p))
        else:
            out.append(ctypes.c_void_p)
    return out


def test_fstat_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in FSTAT_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_fstat_create"] == sig["bflbm_batch_fstat_create"] == sig["bflbm_ring_fstat_create"]
    assert header.count("Field statistics:") == 1
    assert hasattr(pkg, "FieldStats") and "FieldStats" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM, pkg.RingLBM):
        assert hasattr(owner, "field_stats")
    assert hasattr(pkg.analysis, "field_statistics")


def test_fstat_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 8)()
    va, pa = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0)
    calls = {
        "bflbm_fstat_create": lambda: lib.bflbm_fstat_create(None, 0, 1, va, 1, pa, pa, 0, ctypes.byref(h)),
        "bflbm_batch_fstat_create": lambda: lib.bflbm_batch_fstat_create(None, 0, 1, va, 1, pa, pa, 0, ctypes.byref(h)),
        "bflbm_ring_fstat_create": lambda: lib.bflbm_ring_fstat_create(None, 0, 1, va, 1, pa, pa, 0, ctypes.byref(h)),
        "bflbm_fstat_sample": lambda: lib.bflbm_fstat_sample(None),
        "bflbm_fstat_reset": lambda: lib.bflbm_fstat_reset(None),
        "bflbm_fstat_count": lambda: lib.bflbm_fstat_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_fstat_get": lambda: lib.bflbm_fstat_get(None, 1, 0, 0, buf),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_fstat_destroy(None) == 0               # like every destroy of the ABI: nothing to do


def test_variable_names_of_the_sources(pkg):
    from_lattice = pkg.lattice.fstat_variable_names
    assert from_lattice(0) == pkg.plotfile.variable_names(22) and from_lattice(1) == pkg.plotfile.variable_names(9)
    noise = from_lattice(2)
    assert len(noise) == 38 and noise[1] == "fa1" and noise[19 + 4] == "ga4"


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_fstat_kernel_metadata(device_asm):
    """k_fstat_accumulate<NV>, NV = 1 .. 8, and k_fstat_derive: no scratch and no LDS, as include/bflbm.h states."""
    found = kernels(device_asm, r"^_Z\w*?18k_fstat_accumulateILi(\d)EE\w*:")    # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    found += kernels(device_asm, r"^_Z\w*?14k_fstat_derive(E)\w*:")
    assert len(found) == 9
    for m, meta in found:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
        assert re.search(r"; LDSByteSize: 0\b", meta), f"{m.group(0)} uses LDS"
