"""Moment traces, CPU side: analysis.moments_of against the oracle's orc_moments, analysis.moment_record against an int64
computation from the integer moment matrix (tests/moment_sums.py, which shares no construction with it) and against a plain
np.sum, the identities of a record, NaN, the cuts of a record (variances, equipartition, stress series), the C-ABI surface
(declared, exported, bound with the header's argument lists), the null-pointer refusals (which must fail before any device
is touched), the host part of csrc/bflbm_moment.h through a stand-alone program built with the address and
undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels, lds_bytes, scratch_size   # noqa: F401  (device_asm: the listing fixture)

import moment_sums as ms
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

MOMENT_SYMBOLS = ["bflbm_moment_create", "bflbm_batch_moment_create", "bflbm_moment_destroy",
                  "bflbm_moment_sample", "bflbm_moment_reset", "bflbm_moment_count", "bflbm_moment_geometry", "bflbm_moment_read"]
BOX = (5, 33, 70)                                          # nz, ny, nx: two tiles per plane, the last short
LDS_LIMIT = 49152                                          # what DESIGN.md states for k_moment_sums


def _random_populations(seed, shape=BOX):
    """Populations of the size of a mixture's: the weights times a density near 1, with fluctuations of a few per cent."""
    rng = np.random.default_rng(seed)
    w = np.array([1. / 3.] + [1. / 18.] * 6 + [1. / 36.] * 12).reshape(19, 1, 1, 1)
    return (w * (1.0 + 0.05 * rng.standard_normal((19,) + shape)), w * (0.7 + 0.05 * rng.standard_normal((19,) + shape)))


# ---- the per-site transform --------------------------------------------------------------------------------------------------
def test_per_site_moments_equal_the_oracle(pkg, ob):
    f, g = _random_populations(11, (2, 3, 25))
    for pops in (f, g, np.random.default_rng(12).standard_normal((19, 2, 3, 25))):
        got = pkg.analysis.moments_of(pops).reshape(19, -1)
        flat = pops.reshape(19, -1)
        for s in range(flat.shape[1]):
            want = ob.moments(flat[:, s])
            assert np.array_equal(got[:, s], want), (s, np.abs(got[:, s] - want).max())


def test_matrix_of_the_helper_is_the_transform(pkg):
    """The integer matrix reproduces the twin's moments of unit populations, and its rows are orthogonal under the weights
    with the norms the reference lists (LBM_d3q19.H:56-76): what equipartition divides by."""
    m = ms.moment_matrix()
    assert np.array_equal(pkg.analysis.moments_of(np.eye(19)), m.astype(np.float64))
    w = np.array([12] + [2] * 6 + [1] * 12, dtype=np.int64)               # 36 w_i
    gram = (m * w) @ m.T
    assert np.array_equal(gram, np.diag(np.diag(gram)))
    assert np.allclose(np.diag(gram) / 36.0, pkg.analysis.MOMENT_NORMS, rtol=1e-15, atol=0)
    names = pkg.analysis.moment_names()
    assert len(names) == 19 == len(set(names)) and names[:4] == ["rho", "jx", "jy", "jz"] and names[7:10] == ["s_xy", "s_yz", "s_xz"]


# ---- the twin against independent computations -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [BOX, (3, 32, 64), (2, 7, 33)])
def test_twin_on_integer_populations_equals_the_int64_computation(pkg, shape):
    f, g = ms.integer_populations(shape, seed=shape[2])
    got = pkg.analysis.moment_record(f, g)
    want = ms.integer_record(f, g)
    assert got.shape == (95,) and got.dtype == np.float64 and want.dtype == np.int64
    assert np.array_equal(got, want.astype(np.float64)), np.nonzero(got != want)[0]
    assert np.abs(want).max() < 2 ** 53 and len(set(want.tolist())) > 80           # exact in doubles, and the words differ


def test_twin_on_random_doubles_within_the_bound_of_a_recursive_sum(pkg):
    f, g = _random_populations(7)
    terms = pkg.analysis.moment_terms(f, g)                # [95, nz, ny, nx]
    got = pkg.analysis.moment_record(f, g)
    plain = terms.reshape(95, -1).sum(axis=1)
    nsites = BOX[0] * BOX[1] * BOX[2]
    bound = nsites * 2.0 ** -52 * np.abs(terms).reshape(95, -1).sum(axis=1)
    assert (np.abs(got - plain) <= bound).all() and (bound > 0).all()
    assert not np.array_equal(got, plain)                  # the orders do differ: the bound is not vacuous
    # the terms themselves: the squares and the cross products of the moments, each rounded once
    mf, mg = pkg.analysis.moments_of(f), pkg.analysis.moments_of(g)
    assert np.array_equal(terms[:19], mf) and np.array_equal(terms[19:38], mg)
    assert np.array_equal(terms[38:57], mf * mf) and np.array_equal(terms[57:76], mg * mg) and np.array_equal(terms[76:], mf * mg)


# ---- the identities ----------------------------------------------------------------------------------------------------------
def test_identities_of_a_record(pkg):
    an = pkg.analysis
    f, g = _random_populations(3)
    rec = an.moment_record(f, g)
    nsites = BOX[0] * BOX[1] * BOX[2]
    assert (rec[38:76] >= 0).all() and (rec[38:76] > 0).all()
    # rho: the sum of the populations; the density of the mixture
    assert abs(rec[0] - f.sum()) <= nsites * 19 * 2.0 ** -52 * np.abs(f).sum() and abs(rec[19] - g.sum()) <= nsites * 19 * 2.0 ** -52 * np.abs(g).sum()
    # the total fluid's variance from sq_f + 2 cross + sq_g against the variance of mf + mg computed directly
    var_f, var_g, var_t = an.moment_variances(rec, nsites)
    mf, mg = an.moments_of(f).reshape(19, -1), an.moments_of(g).reshape(19, -1)
    for got, m in ((var_f, mf), (var_g, mg), (var_t, mf + mg)):
        direct = m.var(axis=1)
        scale = (m * m).mean(axis=1)                       # the cancellation is against the mean square
        assert (np.abs(got - direct) <= 64 * nsites * 2.0 ** -52 * scale).all(), np.abs(got - direct) / scale
        assert (direct > 0).all()
    # Cauchy-Schwarz: cross^2 <= sq_f sq_g
    assert (rec[76:] ** 2 <= rec[38:57] * rec[57:76] * (1 + 1e-12)).all()
    e_f, e_g, e_t = an.equipartition(rec, nsites)
    for e in (e_f, e_g, e_t):
        assert e.shape == (19,) and abs(e[1:4].mean() - 1.0) < 1e-14
    b = np.array(an.MOMENT_NORMS)
    assert np.allclose(e_f, (var_f / b) / (var_f / b)[1:4].mean(), rtol=1e-15)
    stress = an.stress_series(rec)
    assert stress.shape == (6,) and np.array_equal(stress, rec[4:10] + rec[23:29])
    many = np.stack([rec, 2 * rec, 3 * rec]).reshape(3, 1, 95)             # [count, B, 95] as read() returns it
    assert an.stress_series(many).shape == (3, 1, 6) and an.equipartition(many, nsites)[2].shape == (3, 1, 19)
    assert an.time_correlation(an.stress_series(many)[:, 0, 3:], max_lag=1).shape == (2, 3)


@pytest.mark.parametrize("fluid,i", [(0, 1), (1, 0), (0, 7), (1, 11), (0, 18)])
def test_nan_shows_in_exactly_the_words_its_moments_enter(pkg, fluid, i):
    f, g = _random_populations(5)
    (f, g)[fluid][i, 2, 17, 41] = np.nan
    rec = pkg.analysis.moment_record(f, g)
    assert np.nonzero(np.isnan(rec))[0].tolist() == ms.words_of_population(fluid, i)
    assert 0 < np.isnan(rec).sum() < 95


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((19, 2, 2, 2))
    for bad in (lambda: an.moment_record(f[:18], f[:18]), lambda: an.moment_record(f, f[:, :1]), lambda: an.moment_record(f[:, 0], f[:, 0]),
                lambda: an.moments_of(np.zeros((18, 4))), lambda: an.moment_variances(np.zeros(94), 8), lambda: an.moment_variances(np.zeros(95), 0),
                lambda: an.equipartition(np.zeros((2, 96)), 8), lambda: an.stress_series(np.zeros(38))):
        with pytest.raises(ValueError):
            bad()


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_moment_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in MOMENT_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_moment_create"] == sig["bflbm_batch_moment_create"]
    create = sig["bflbm_moment_create"][1]                 # (owner, every, capacity, out)
    assert len(create) == 4 and create[1] is ctypes.c_int and create[2] is ctypes.c_longlong
    assert len(sig["bflbm_moment_geometry"][1]) == 4 and sig["bflbm_moment_read"][1][3] is ctypes.c_void_p
    assert header.count("Moment traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert hasattr(pkg, "MomentTrace") and "MomentTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "moment_trace")
    assert "bflbm_ring_moment_create" not in sig and not hasattr(lib, "bflbm_ring_moment_create") and not hasattr(pkg.RingLBM, "moment_trace")   # a ring is not built
    for fn in ("moment_record", "moment_terms", "moments_of", "moment_names", "moment_variances", "equipartition", "stress_series", "time_correlation"):
        assert hasattr(pkg.analysis, fn)
    block = header[header.index("Moment traces:"):header.index("typedef struct bflbm_moment")]
    for words in ("mf = moments(f) and mg = moments(g)", "fold / gold", "i = 19 fluid + a", "fa0..fa18, ga0..ga18", "W = 95 doubles",
                  "sum[i] (words 0..37)", "sq[i] (words\n *    38..75)", "cross[a] (words 76..94)", "rounded once and then added", "-ffp-contract=off",
                  "A NaN\n *    stays in its sum", "the lag trace's order for `now`", "no variable lists and no pair\n *    lists",
                  "the record depends on the box alone", "bit for bit", "no bflbm_ring_moment_create", "it is not built", "compile-time index",
                  "49152 bytes of\n *    static LDS", "[replica][z][95][tiles]", "No atomics, no scratch", "304 bytes read against the 608 of a step",
                  "95 x tiles partials per plane", "what is touched on the owner: nothing", "\"moment\n *    trace full\"",
                  "arbitrary pairs of modes", "a Green-Kubo integral"):
        assert words in block, words
    kernel_header = open(os.path.join(CSRC, "bflbm_moment.h")).read()
    for words in ("derived, not measured", "304 bytes read", "ScratchSize 0", "49152 bytes of static LDS", "nothing of the owner written", "no bflbm_ring_moment_create", "It is not built"):
        assert words in kernel_header, words
    assert "moment traces (bflbm_moment.h)" in open(os.path.join(CSRC, "bflbm_recorder.h")).read()
    assert "bflbm_moment" not in open(os.path.join(CSRC, "bflbm_fieldsel.h")).read()       # no new source in the field selection


def test_moment_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 95)()
    g = [ctypes.c_int() for _ in range(3)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 1, 4, ctypes.byref(h))) for name in MOMENT_SYMBOLS[:2]}
    calls.update({
        "bflbm_moment_sample": lambda: lib.bflbm_moment_sample(None),
        "bflbm_moment_reset": lambda: lib.bflbm_moment_reset(None),
        "bflbm_moment_count": lambda: lib.bflbm_moment_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_moment_geometry": lambda: lib.bflbm_moment_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_moment_read": lambda: lib.bflbm_moment_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    owner = ctypes.cast(buf, ctypes.c_void_p)              # a null result is refused before the owner is looked at
    for name in MOMENT_SYMBOLS[:2]:
        assert getattr(lib, name)(owner, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_moment_destroy(None) == 0             # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_layout_tiles_refusals_and_launch_shapes_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "moment_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "moment_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 39  # the checks moment_main.cpp makes: a check that silently stops running fails here


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_moment_kernel_metadata(device_asm):
    """k_moment_sums<false> and <true>: no scratch in either instantiation, as include/bflbm.h states, and the static LDS of the
    tree's two buffers within the limit DESIGN.md states.  With the finishing launch: 3 kernels."""
    found = kernels(device_asm, r"^_Z\w*?13k_moment_sumsILb([01])EE\w*:")                # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == [0, 1]
    for m, meta in found:
        assert scratch_size(meta) == 0, f"{m.group(0)} spills to scratch"
        assert 0 < lds_bytes(meta) <= LDS_LIMIT, f"{m.group(0)}: static LDS {lds_bytes(meta)}"
    finish = kernels(device_asm, r"^_Z\w*?15k_moment_finish\w*:")
    assert len(finish) == 1 and scratch_size(finish[0][1]) == 0
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_moment_\w*:")) == 3
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d bytes of static LDS" % LDS_LIMIT in design and "k_moment_sums" in design
