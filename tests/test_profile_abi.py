"""Profile traces, CPU side: analysis.plane_profiles against the exact plane sums and the site-by-site emulation of the
kernels' order (tests/profile_sums.py), analysis.pressure_profile and mechanical_surface_tension on a tanh profile
with a closed form, the C-ABI surface (declared, exported, bound with the header's argument lists), the null-pointer
refusals (which must fail before any device is touched) and the compiled kernels' metadata (hipcc cross-compiles
gfx950, no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import profile_sums as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROFILE_SYMBOLS = ["bflbm_profile_create", "bflbm_batch_profile_create", "bflbm_ring_profile_create", "bflbm_profile_destroy",
                   "bflbm_profile_sample", "bflbm_profile_reset", "bflbm_profile_count", "bflbm_profile_geometry",
                   "bflbm_profile_read"]
PAIRS = [(0, 1), (2, 2), (1, 0)]


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["x", "y", "z"])
@pytest.mark.parametrize("n", ps.BOXES)
def test_plane_profiles_against_the_exact_sums_and_the_emulation(pkg, n, axis):
    """Random fields of both signs (so that the sums cancel): the twin equals the site-by-site emulation bit for bit and
    lies inside depth_bound * sum |term| of the exact sums."""
    nx, ny, nz = n
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    fields = rng.standard_normal((3, nz, ny, nx)) * np.exp(rng.uniform(-3, 3, size=(3, nz, ny, nx)))
    got = pkg.analysis.plane_profiles(fields, PAIRS, axis)
    assert got.shape == (6, n[ps.AXES[axis]]) and got.dtype == np.float64
    assert np.array_equal(got, ps.emulate(fields, PAIRS, axis)), (n, axis)
    bound = ps.depth_bound(nx, ny, nz, axis)
    worst = ps.ratio_to_bound(got, ps.exact(fields, PAIRS, axis), ps.abs_sums(fields, PAIRS, axis), bound)
    print(n, axis, "worst |twin - exact| / (depth_bound sum |term|) = %.3g, depth_bound = %.3g" % (worst, bound))
    assert worst <= 1.0, (n, axis, worst)
    assert np.array_equal(pkg.analysis.plane_profiles(fields, PAIRS, ps.AXES[axis]), got)     # the axis by number


def test_plane_profiles_refuses_bad_arguments(pkg):
    f = np.zeros((2, 3, 4, 5))
    for bad in (lambda: pkg.analysis.plane_profiles(f, [(0, 2)], "z"), lambda: pkg.analysis.plane_profiles(f, [], 3),
                lambda: pkg.analysis.plane_profiles(f[0], [], "z")):
        with pytest.raises(ValueError):
            bad()
    assert pkg.analysis.plane_profiles(f, [], "x").shape == (2, 5)


# ---- the pressure profile --------------------------------------------------------------------------------------------------
def _tanh_means(axis, alpha0, cs2, n=64, w=2.0, A=1.4, B=1.1):
    """The plane means of one flat interface along `axis` made by hand: rho = 1.6 + A tanh(s / w), phi = 1.5 - B tanh(s / w)
    at the plane centres s = i + 1/2 - n/2, with the analytic gradients in af = -cs2 alpha0 grad phi and
    ag = -cs2 alpha0 grad rho, uniform in every plane (so <a b> = a b) and no tangential gradient."""
    variables, pairs = ("rho phi afx afy afz agx agy agz".split(), [("rho", "phi"), ("afx", "agx"), ("afy", "agy"), ("afz", "agz")])
    s = np.arange(n) + 0.5 - n / 2
    sech2 = 1.0 / np.cosh(s / w) ** 2
    rho, phi = 1.6 + A * np.tanh(s / w), 1.5 - B * np.tanh(s / w)
    drho, dphi = A / w * sech2, -B / w * sech2
    val = {v: np.zeros(n) for v in variables}
    val["rho"], val["phi"] = rho, phi
    val["af" + "xyz"[axis]], val["ag" + "xyz"[axis]] = -cs2 * alpha0 * dphi, -cs2 * alpha0 * drho
    means = np.array([val[v] for v in variables] + [val[a] * val[b] for a, b in pairs])
    return means, variables, pairs, (rho, phi)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pressure_profile_and_surface_tension_of_a_tanh_profile(pkg, axis):
    """-alpha0 cs^4 integral rho' phi' ds = alpha0 cs^4 A B / w^2 integral sech^4(s / w) ds = 4 alpha0 cs^4 A B / (3 w).
    The test sums f(s) = sech^4(s / w) at the n = 64 midpoints s = i + 1/2 - 32 instead.  Poisson's summation formula:
    sum over all integers i of f(i + 1/2) = sum over m of (-1)^m F(2 pi m), F(k) = integral f(s) e^{-iks} ds =
    w pi kw (4 + (kw)^2) / (6 sinh(pi kw / 2)) (F(0) = 4 w / 3 is the integral), so the midpoint sum over the whole line
    misses the integral by at most 2 sum_{m >= 1} |F(2 pi m)|; the planes left out beyond |s| > 32 hold at most
    integral_{31.5}^inf 16 e^{-4 s / w} ds each side (sech <= 2 e^{-|x|}, f decreasing); rounding adds some 64 u.  With
    w = 2 the first is 4.1e-6 of the integral: a tolerance the arithmetic of the function can miss."""
    alpha0, cs2, w, A, B, n = 1.7, 1.0 / 3.0, 2.0, 1.4, 1.1, 64
    means, names, pairs, (rho, phi) = _tanh_means(axis, alpha0, cs2, n, w, A, B)
    p_bulk, pnt = pkg.analysis.pressure_profile(means, names, alpha0, cs2, axis)
    assert p_bulk.shape == (n,) and pnt.shape == (n,)
    assert np.allclose(p_bulk, cs2 * (rho + phi) + alpha0 * cs2 * rho * phi, rtol=4e-16, atol=0)
    assert (pnt > 0).all()                                 # rho' phi' < 0 across this interface: P_N > P_T, gamma > 0
    gamma = pkg.analysis.mechanical_surface_tension(pnt, interfaces=1)
    closed = 4.0 * alpha0 * cs2 ** 2 * A * B / (3.0 * w)

    def F(k):
        return w * math.pi * k * w * (4.0 + (k * w) ** 2) / (6.0 * math.sinh(math.pi * k * w / 2.0))
    poisson = 2.0 * sum(F(2.0 * math.pi * m) for m in range(1, 6))
    tails = 2.0 * 16.0 * (w / 4.0) * math.exp(-4.0 * (n / 2 - 0.5) / w)
    tol = (poisson + tails) / (4.0 * w / 3.0) * 1.001 + 256 * np.finfo(np.float64).eps
    print("axis %d: gamma %.15g, closed form %.15g, relative difference %.3g, tolerance %.3g" % (axis, gamma, closed, abs(gamma / closed - 1), tol))
    assert tol < 1e-5 and abs(gamma / closed - 1.0) <= tol
    # the tensor is read along the named axis only: another normal sees no gradient there and a tangential one instead
    other = pkg.analysis.pressure_profile(means, names, alpha0, cs2, (axis + 1) % 3)[1]
    assert np.allclose(other, -0.5 * pnt, rtol=1e-15, atol=0)
    # two interfaces halve the sum; the means may carry leading axes [count, B]
    stacked = np.broadcast_to(means, (2, 3) + means.shape)
    pb2, pnt2 = pkg.analysis.pressure_profile(stacked, names, alpha0, cs2, "xyz"[axis])
    assert pb2.shape == (2, 3, n) and np.array_equal(pnt2[1, 2], pnt)
    assert np.allclose(pkg.analysis.mechanical_surface_tension(pnt2), np.full((2, 3), gamma / 2.0), rtol=1e-15, atol=0)


def test_pressure_profile_inputs_and_refusals(pkg):
    an = pkg.analysis
    variables, pairs = an.pressure_profile_inputs()
    assert variables == "rho phi afx afy afz agx agy agz".split()
    assert pairs == [("rho", "phi"), ("afx", "agx"), ("afy", "agy"), ("afz", "agz")]
    assert all(v in pkg.plotfile.variable_names(22) for v in variables)
    means, names, _, _ = _tanh_means(2, 1.5, 1.0 / 3.0)
    with pytest.raises(ValueError, match="alpha0 == 0"):
        an.pressure_profile(means, names, 0.0, 1.0 / 3.0, 2)
    with pytest.raises(ValueError, match="'agz' is missing"):
        an.pressure_profile(means[[0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11]], names[:7], 1.5, 1.0 / 3.0, 2)
    with pytest.raises(ValueError, match="afy agy is missing"):
        an.pressure_profile(means[:11], names, 1.5, 1.0 / 3.0, 2, pairs=[pairs[0], pairs[1], pairs[3]])
    with pytest.raises(ValueError, match="Q = 8 variables"):
        an.pressure_profile(means[:11], names, 1.5, 1.0 / 3.0, 2)
    with pytest.raises(ValueError, match="axis"):
        an.pressure_profile(means, names, 1.5, 1.0 / 3.0, 3)
    # pairs in another order and by slot
    order = [3, 0, 2, 1]
    shuffled = np.concatenate([means[:8], means[8:][order]])
    want = an.pressure_profile(means, names, 1.5, 1.0 / 3.0, 2)
    got = an.pressure_profile(shuffled, names, 1.5, 1.0 / 3.0, 2, pairs=[(7, 4), ("phi", "rho"), ("agy", "afy"), (2, 5)])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


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


def test_profile_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in PROFILE_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_profile_create"] == sig["bflbm_batch_profile_create"] == sig["bflbm_ring_profile_create"]
    # (owner, source, axis, nvars, vars, npairs, pair_a, pair_b, every, capacity, out)
    assert len(sig["bflbm_profile_create"][1]) == 11 and sig["bflbm_profile_create"][1][9] is ctypes.c_longlong
    assert header.count("Profile traces:") == 1
    assert hasattr(pkg, "ProfileTrace") and "ProfileTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM, pkg.RingLBM):
        assert hasattr(owner, "profile_trace")
    for fn in ("plane_profiles", "pressure_profile", "mechanical_surface_tension", "pressure_profile_inputs"):
        assert hasattr(pkg.analysis, fn)
    # the header, the numpy twin and the tests' emulation state the same constants
    an = pkg.analysis
    assert (an.PROFILE_TILE, an.PROFILE_LANES, an.PROFILE_CHUNK) == (ps.TILE, ps.LANES, ps.CHUNK) == (2048, 64, 64)
    block = header[header.index("Profile traces:"):header.index("typedef struct bflbm_profile")]
    assert "tiles of 2048 consecutive sites" in block and "lane l of 64" in block and "chunks of 64" in block


def test_profile_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 8)()
    va, pa = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0)
    g = [ctypes.c_int() for _ in range(4)]
    calls = {
        "bflbm_profile_create": lambda: lib.bflbm_profile_create(None, 0, 2, 1, va, 1, pa, pa, 1, 4, ctypes.byref(h)),
        "bflbm_batch_profile_create": lambda: lib.bflbm_batch_profile_create(None, 0, 2, 1, va, 1, pa, pa, 1, 4, ctypes.byref(h)),
        "bflbm_ring_profile_create": lambda: lib.bflbm_ring_profile_create(None, 0, 2, 1, va, 1, pa, pa, 1, 4, ctypes.byref(h)),
        "bflbm_profile_sample": lambda: lib.bflbm_profile_sample(None),
        "bflbm_profile_reset": lambda: lib.bflbm_profile_reset(None),
        "bflbm_profile_count": lambda: lib.bflbm_profile_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_profile_geometry": lambda: lib.bflbm_profile_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_profile_read": lambda: lib.bflbm_profile_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_profile_destroy(None) == 0             # like every destroy of the ABI: nothing to do


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_profile_kernel_metadata(device_asm):
    """k_profile_planes<NV>, NV = 1 .. 8, and k_profile_finish: no scratch; the plane kernel's LDS is the 1536 (NV + 16)
    bytes include/bflbm.h states, the finishing kernel uses none."""
    found = kernels(device_asm, r"^_Z\w*?16k_profile_planesILi(\d)EE\w*:")      # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        assert re.search(r"; LDSByteSize: %d\b" % (1536 * (int(m.group(1)) + 16)), meta), f"{m.group(0)}: LDS"
    finish = kernels(device_asm, r"^_Z\w*?16k_profile_finish(E)\w*:")
    assert len(finish) == 1 and re.search(r"; LDSByteSize: 0\b", finish[0][1])
    for m, meta in found + finish:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
