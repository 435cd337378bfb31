"""Lag traces, CPU side: analysis.lag_record against a plain per-origin loop over np.sum and a site-by-site persistence walk
(which share no construction with it), analysis.lag_slots against a plain loop, the identities of a record, NaN and the level
itself, the averages over origins, the C-ABI surface (declared, exported, bound with the header's argument lists), the
null-pointer refusals (which must fail before any device is touched), the host part of csrc/bflbm_lag.h through a stand-alone
program built with the address and undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc cross-compiles
gfx950, no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

LAG_SYMBOLS = ["bflbm_lag_create", "bflbm_batch_lag_create", "bflbm_lag_destroy", "bflbm_lag_sample", "bflbm_lag_reset",
               "bflbm_lag_count", "bflbm_lag_geometry", "bflbm_lag_read"]
SCHEDULES = [(1, 1, 5), (3, 2, 8), (16, 1, 8), (2, 3, 20)]      # R, E, samples
PAIRS = [(0, 0), (0, 1), (2, 1)]
BOX = (5, 33, 70)                                          # nz, ny, nx: two tiles per plane, the last short


def _plain_slots(ns, r, e):
    """Which sample's origin every slot holds at every sample, by walking the samples."""
    held, now, nxt = [], [-1] * r, 0
    for n in range(ns):
        if n % e == 0:
            now[nxt] = n
            nxt = (nxt + 1) % r
        held.append(list(now))
    return held


def _plain_record(frames, steps, pairs, r, e, ps, level):
    """The record by a per-origin Python loop over np.sum (any order of summation) and a site-by-site persistence walk."""
    ns, nv = frames.shape[:2]
    held = _plain_slots(ns, r, e)
    now = np.array([[np.sum(frames[n, v]) for v in range(nv)] for n in range(ns)])
    osteps = np.full((ns, r), -1, dtype=np.int64)
    alive = np.full((ns, r), -1, dtype=np.int64)
    corr = np.full((ns, r, len(pairs)), np.nan)
    bound = np.zeros((ns, r, len(pairs)))
    bit = {}
    for n in range(ns):
        for k in range(r):
            o = held[n][k]
            if o < 0:
                continue
            osteps[n, k] = steps[o]
            for p, (a, b) in enumerate(pairs):
                terms = frames[n, a] * frames[o, b]
                corr[n, k, p] = np.sum(terms)
                bound[n, k, p] = terms.size * 2.0 ** -52 * np.sum(np.abs(terms))
            if ps >= 0:
                count = 0
                for site in np.ndindex(*frames.shape[2:]):
                    if o == n:
                        bit[k, site] = True
                    v, w = frames[(n, ps) + site], frames[(o, ps) + site]
                    bit[k, site] = bit[k, site] and ((v >= level) == (w >= level))
                    count += bit[k, site]
                alive[n, k] = count
    return now, osteps, alive, corr, bound


# ---- the slot schedule -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,e,ns", SCHEDULES)
def test_lag_slots_against_a_plain_loop(pkg, r, e, ns):
    got = pkg.analysis.lag_slots(ns, r, e)
    assert got.dtype == np.int64 and got.tolist() == _plain_slots(ns, r, e)
    assert (got[:, 0] >= 0).all() and got[0].tolist() == [0] + [-1] * (r - 1)      # sample 0 takes slot 0
    assert pkg.analysis.lag_slots(0, r, e).shape == (0, r)


def test_lag_slots_refuses_bad_arguments(pkg):
    for bad in ((-1, 1, 1), (4, 0, 1), (4, 17, 1), (4, 1, 0)):
        with pytest.raises(ValueError):
            pkg.analysis.lag_slots(*bad)
    assert pkg.analysis.lag_slots(3, 16, 1).shape == (3, 16)
    assert (pkg.analysis.LAG_MAX_VARS, pkg.analysis.LAG_MAX_PAIRS, pkg.analysis.LAG_MAX_ORIGINS) == (8, 8, 16)


# ---- the twin against an independent count -----------------------------------------------------------------------------------
@pytest.mark.parametrize("r,e", [(1, 1), (3, 2), (16, 1)])
def test_twin_on_integer_fields_equals_the_plain_loop(pkg, r, e):
    """Small integers: every product and every partial sum is an integer below 2^53, so every order gives the same double."""
    rng = np.random.default_rng(100 * r + e)
    frames = rng.integers(-9, 10, size=(8, 3, 2, 5, 7)).astype(np.float64)
    steps = np.arange(8, dtype=np.int64) * 3 + 11
    got = pkg.analysis.lag_record(frames, steps, PAIRS, r, e, 1, 0.0)
    want = _plain_record(frames, steps, PAIRS, r, e, 1, 0.0)
    for g, w in zip(got, want[:4]):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype == np.float64)
    assert got[1].dtype == np.int64 and got[2].dtype == np.int64 and got[3].shape == (8, r, 3)
    off = pkg.analysis.lag_record(frames, steps, PAIRS, r, e)           # no persistence: the same sums, alive -1
    assert (off[2] == -1).all() and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(off[:2] + off[3:], got[:2] + got[3:]))


def test_twin_on_random_doubles_within_the_bound_of_a_recursive_sum(pkg):
    rng = np.random.default_rng(7)
    frames = rng.standard_normal((6, 3) + BOX) + 0.25
    steps = np.arange(6, dtype=np.int64) * 5
    now, osteps, alive, corr = pkg.analysis.lag_record(frames, steps, PAIRS, 3, 2, 2, 0.25)
    p_now, p_osteps, p_alive, p_corr, bound = _plain_record(frames, steps, PAIRS, 3, 2, 2, 0.25)
    assert np.array_equal(osteps, p_osteps) and np.array_equal(alive, p_alive)
    nsites = BOX[0] * BOX[1] * BOX[2]
    assert (np.abs(now - p_now) <= nsites * 2.0 ** -52 * np.abs(frames).sum(axis=(2, 3, 4))).all()
    held = np.isfinite(p_corr)
    assert np.array_equal(held, np.isfinite(corr)) and held.sum() == (1 + 1 + 2 + 2 + 3 + 3) * 3      # origins at the samples 0, 2, 4
    assert (np.abs(corr - p_corr)[held] <= bound[held]).all() and (bound[held] > 0).all()
    assert not np.array_equal(corr[held], p_corr[held])    # the orders do differ: the bound is not vacuous


# ---- the identities ----------------------------------------------------------------------------------------------------------
def test_identities_of_a_record(pkg):
    an = pkg.analysis
    rng = np.random.default_rng(3)
    frames = rng.standard_normal((8, 2) + BOX)
    steps = np.arange(8, dtype=np.int64) + 1
    pairs = [(0, 1), (1, 1)]
    now, osteps, alive, corr = an.lag_record(frames, steps, pairs, 3, 2, 0, 0.0)
    held = an.lag_slots(8, 3, 2)
    nsites = BOX[0] * BOX[1] * BOX[2]
    for n in range(8):
        prof = an.plane_profiles(frames[n], pairs, axis=2)                 # [Q, nz]
        total = np.zeros(4)
        for z in range(BOX[0]):
            total = total + prof[:, z]
        assert np.array_equal(now[n], total[:2])
        for k in range(3):
            if held[n, k] == n:                            # lag 0: the profile trace's own pairs; every bit set
                assert np.array_equal(corr[n, k], total[2:]) and alive[n, k] == nsites and osteps[n, k] == steps[n]
            if n > 0 and held[n, k] >= 0 and held[n, k] == held[n - 1, k]:
                assert alive[n, k] <= alive[n - 1, k]      # within an origin, alive does not increase
    assert (alive[held >= 0] > 0).all() and (alive[held >= 0] < nsites).sum() > 0 and (alive[held < 0] == -1).all()
    assert np.isnan(corr[held < 0]).all() and (osteps[held < 0] == -1).all() and (held < 0).sum() == 2 + 2 + 1 + 1
    # a site that crosses and returns between two samples stays alive: P depends on `every`
    f = np.ones((3, 1, 1, 1, 4))
    f[1, 0, 0, 0, 2] = -1.0
    assert an.lag_record(f, [0, 1, 2], [(0, 0)], 1, 8, 0, 0.0)[2][:, 0].tolist() == [4, 3, 3]
    assert an.lag_record(f[::2], [0, 2], [(0, 0)], 1, 8, 0, 0.0)[2][:, 0].tolist() == [4, 4]


def test_nan_and_the_level_itself(pkg):
    an = pkg.analysis
    rng = np.random.default_rng(5)
    frames = np.abs(rng.standard_normal((3, 2, 2, 3, 4))) + 1.0          # everything above the level 1.0
    frames[0, 0, 0, 0, 0] = 1.0                                          # equal to the level: above
    frames[1, 0, 1, 2, 3] = np.nan                                       # a NaN in the second frame: false, so it crossed
    now, osteps, alive, corr = an.lag_record(frames, [0, 1, 2], [(0, 0), (0, 1), (1, 0), (1, 1)], 2, 1, 0, 1.0)
    assert alive[:, 0].tolist() == [24, 23, 24]            # the NaN's site has crossed; the site at the level has not; sample 2 takes slot 0 again
    assert alive[:, 1].tolist() == [-1, 24, 23]            # a NaN at the origin is on the false side: itself at lag 0, crossed later
    assert an.lag_record(frames, [0, 1, 2], [(0, 0)], 1, 8, 0, 1.0)[2][:, 0].tolist() == [24, 23, 23]      # one origin: dead for good
    assert np.isnan(now[1, 0]) and np.isfinite(now[[0, 2]]).all() and np.isfinite(now[:, 1]).all()
    # sample 1: the NaN is in a(now) of the pairs 0, 1 for both slots, and in b(origin 1) of the pairs 0, 2
    assert np.isnan(corr[1, 0]).tolist() == [True, True, False, False] and np.isnan(corr[1, 1]).tolist() == [True, True, True, False]
    # sample 2: only the origin of slot 1 carries it
    assert np.isnan(corr[2, 0]).tolist() == [False] * 4 and np.isnan(corr[2, 1]).tolist() == [True, False, True, False]
    below = frames.copy()
    below[0, 0, 0, 0, 0] = np.nextafter(1.0, 0.0)                        # just below: it crosses at sample 1
    assert an.lag_record(below, [0, 1, 2], [(0, 0)], 1, 8, 0, 1.0)[2][:, 0].tolist() == [24, 22, 22]


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((2, 2, 2, 2, 2))
    for bad in (lambda: an.lag_record(f[0], [0, 1], [(0, 0)], 1), lambda: an.lag_record(np.zeros((2, 9, 1, 1, 1)), [0, 1], [(0, 0)], 1),
                lambda: an.lag_record(f, [0], [(0, 0)], 1), lambda: an.lag_record(f, [0, 1], [], 1), lambda: an.lag_record(f, [0, 1], [(0, 0)] * 9, 1),
                lambda: an.lag_record(f, [0, 1], [(0, 2)], 1), lambda: an.lag_record(f, [0, 1], [(0, 0)], 0), lambda: an.lag_record(f, [0, 1], [(0, 0)], 17),
                lambda: an.lag_record(f, [0, 1], [(0, 0)], 1, 0), lambda: an.lag_record(f, [0, 1], [(0, 0)], 1, 1, 2, 0.0),
                lambda: an.lag_record(f, [0, 1], [(0, 0)], 1, 1, -2, 0.0), lambda: an.lag_record(f, [0, 1], [(0, 0)], 1, 1, 0, np.inf),
                lambda: an.lag_average([0, 1], np.zeros((2, 3)), np.zeros((2, 2))), lambda: an.lag_average([0], np.zeros((2, 3)), np.zeros((2, 3))),
                lambda: an.lag_connected([0, 1], np.zeros((2, 3)), np.zeros((2, 3)), [0.0], [0.0, 1.0], 8),
                lambda: an.lag_connected([0, 1], np.zeros((2, 3)), np.zeros((2, 3)), [0.0, 1.0], [0.0, 1.0], 0)):
        with pytest.raises(ValueError):
            bad()


# ---- the averages over origins -----------------------------------------------------------------------------------------------
def test_average_and_connected_part(pkg):
    an = pkg.analysis
    steps = np.array([10, 13, 16, 19], dtype=np.int64)
    held = an.lag_slots(4, 2, 1)                           # slots: [0,-] [0,1] [2,1] [2,3]
    osteps = np.where(held >= 0, steps[np.maximum(held, 0)], -1)
    values = np.where(held >= 0, (steps[:, None] - osteps) * 1.0 + 100.0 * np.maximum(held, 0), np.nan)
    lags, mean, count = an.lag_average(steps, osteps, values)
    assert lags.tolist() == [0, 3] and count.tolist() == [4, 3] and count.dtype == np.int64
    assert mean.tolist() == [(0 + 100 + 200 + 300) / 4.0, (3 + 103 + 203) / 3.0]
    # a constant field c: corr = nsites c^2 and now = nsites c, so the connected part vanishes where the origin's sample is in the record
    c, nsites = 1.5, 64
    corr = np.where(held >= 0, nsites * c * c, np.nan)
    now = np.full(4, nsites * c)
    conn = an.lag_connected(steps, osteps, corr, now, now, nsites)
    assert np.array_equal(np.isnan(conn), held < 0) and (conn[held >= 0] == 0.0).all()
    # a window without the first sample: the origin of step 10 is not in the record any more
    window = an.lag_connected(steps[1:], osteps[1:], corr[1:], now[1:], now[1:], nsites)
    assert np.isnan(window[0, 0]) and window[0, 1] == 0.0 and np.isfinite(window[1:]).all()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_lag_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in LAG_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_lag_create"] == sig["bflbm_batch_lag_create"]
    # (owner, source, nvars, vars, npairs, pair_a, pair_b, norigins, origin_stride, persist_slot, persist_level, every, capacity, out)
    create = sig["bflbm_lag_create"][1]
    assert len(create) == 14 and create[10] is ctypes.c_double and create[12] is ctypes.c_longlong
    assert sig["bflbm_lag_read"][1][3] is ctypes.c_void_p                               # 8-byte words
    geo = sig["bflbm_lag_geometry"][1]
    assert len(geo) == 10 and geo[8] == ctypes.POINTER(ctypes.c_longlong) and geo[9] == ctypes.POINTER(ctypes.c_longlong)
    assert header.count("Lag traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert "bflbm_ring_lag_create" not in sig and not hasattr(lib, "bflbm_ring_lag_create")            # a ring is not built
    assert hasattr(pkg, "LagTrace") and "LagTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "lag_trace")
    assert not hasattr(pkg.RingLBM, "lag_trace")
    for fn in ("lag_slots", "lag_record", "lag_average", "lag_connected"):
        assert hasattr(pkg.analysis, fn)
    # the header states the rule, the limits and what is not built; the kernel's header says why there is no ring
    block = header[header.index("Lag traces:"):header.index("typedef struct bflbm_lag")]
    for words in ("nvars in 1..8", "npairs in 1..8", "norigins R in 1..16", "origin_stride E >= 1", "n % E == 0", "(n / E) % R",
                  "every origin appears at lag 0", "W = nvars + R (2 + npairs)", "-1 while the slot is empty", "NaN for an\n *    empty slot",
                  "rounded once and then added", "A NaN in a field propagates", "a NaN gives false", "equal to the level\n *    is above",
                  "s(v now) == s(v at origin r)", "P depends on `every`", "tiles\n *    of 2048 consecutive dense sites", "w = 128 .. 1",
                  "z = 0 .. nz-1, from +0.0", "bit for bit", "No atomics\n *    on doubles, no scratch, no grid barrier", "8 nvars (1 + L)",
                  "408 bytes", "no bflbm_ring_lag_create", "it is not built", "logarithmically spaced origins", "per-site lagged products",
                  "\"lag trace\n *    full\"", "also empties the slots and restarts n"):
        assert words in block, words
    kernel_header = open(os.path.join(CSRC, "bflbm_lag.h")).read()
    for words in ("no bflbm_ring_lag_create", "It is not built", "derived, not measured", "8 nvars (1 + L) bytes read", "ScratchSize 0"):
        assert words in kernel_header, words
    assert "lag traces (bflbm_lag.h)" in open(os.path.join(CSRC, "bflbm_recorder.h")).read()


def test_lag_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 16)()
    va = (ctypes.c_int * 1)(0)
    g = [ctypes.c_int() for _ in range(7)] + [ctypes.c_longlong() for _ in range(2)]
    tail = (8, 1, -1, 0.0, 1, 4)
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 1, va, 1, va, va, *tail, ctypes.byref(h))) for name in LAG_SYMBOLS[:2]}
    calls.update({
        "bflbm_lag_sample": lambda: lib.bflbm_lag_sample(None),
        "bflbm_lag_reset": lambda: lib.bflbm_lag_reset(None),
        "bflbm_lag_count": lambda: lib.bflbm_lag_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_lag_geometry": lambda: lib.bflbm_lag_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_lag_read": lambda: lib.bflbm_lag_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null array and a null result are refused before the owner is looked at: any non-null pointer will do
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in LAG_SYMBOLS[:2]:
        for args in ((None, 1, va, va), (va, 1, None, va), (va, 1, va, None)):
            assert getattr(lib, name)(owner, 0, 1, *args, *tail, ctypes.byref(h)) != 0
            assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 1, va, 1, va, va, *tail, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_lag_destroy(None) == 0                # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_layout_schedule_refusals_and_launch_shapes_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "lag_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "lag_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 102  # the checks lag_main.cpp makes: a check that silently stops running fails here


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_lag_kernel_metadata(device_asm):
    """k_lag_products<NV>, NV = 1 .. 8: no scratch in any instantiation, as include/bflbm.h states, and the static LDS of the
    tree (two buffers of 8 x 256 doubles) and of the 16 wave counters.  With the labelling and the two finishing launches: 11 kernels."""
    found = kernels(device_asm, r"^_Z\w*?14k_lag_productsILi(\d)EE\w*:")                # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
        assert re.search(r"; LDSByteSize: 32832\b", meta), f"{m.group(0)}: static LDS"
    others = kernels(device_asm, r"^_Z\w*?\d+k_lag_(label|planes|finish)\w*:")
    assert sorted(m.group(1) for m, _ in others) == ["finish", "label", "planes"]
    for m, meta in others:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_lag_\w*:")) == 11
