"""Radial traces, CPU side: analysis.radial_shells against the site-by-site emulation of the kernels' order and the exact
sums (tests/radial_sums.py), the pair and radial terms and the Laplace-law helpers on a tanh droplet made by hand, the
physics of the four golden droplets (tests/golden/radial_droplets.npz) against the numbers Surface_Tension.ipynb records,
the C-ABI surface (declared, exported, bound with the header's argument lists), the null-pointer refusals (which must
fail before any device is touched) and the compiled kernels' metadata (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import radial_sums as rs
from test_gpu_notebook_surface_tension import CELL13, CELL18, GAMMA_15, GAMMA_17, R_15, R_17

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "radial_droplets.npz")

RADIAL_SYMBOLS = ["bflbm_radial_create", "bflbm_batch_radial_create", "bflbm_radial_destroy", "bflbm_radial_sample",
                  "bflbm_radial_reset", "bflbm_radial_count", "bflbm_radial_geometry", "bflbm_radial_read"]
PAIRS = [(0, 1), (2, 2), (1, 0)]
RADIALS = [(None, (0, 1, 2)), (1, (2, 0, 1))]
DELTA = 0.75


def _random_fields(n):
    nx, ny, nz = n
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    return rng.standard_normal((3, nz, ny, nx)) * np.exp(rng.uniform(-3, 3, size=(3, nz, ny, nx)))


# ---- the numpy twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["corner", "integer", "half", "nan"])
@pytest.mark.parametrize("n", rs.BOXES)
def test_radial_shells_against_the_emulation_and_the_exact_sums(pkg, n, which):
    """Random fields of both signs (so that the sums cancel): the twin equals the site-by-site emulation bit for bit and
    lies inside depth_bound * sum |term| of the exact sums of the rounded terms, with shells that cover the box and with
    three shells only."""
    fields, centre = _random_fields(n), rs.centres(n)[which]
    nsites = n[0] * n[1] * n[2]
    for nbins in (rs.default_bins(n, DELTA), 3):
        counts, sums = pkg.analysis.radial_shells(fields, centre, DELTA, nbins, PAIRS, RADIALS)
        assert counts.shape == (nbins,) and sums.shape == (8, nbins) and sums.dtype == np.float64
        want = rs.emulate(fields, centre, DELTA, nbins, PAIRS, RADIALS)
        assert np.array_equal(counts, want[0]) and np.array_equal(sums, want[1]), (n, which, nbins)
        got = np.concatenate([counts[None], sums])
        bound = rs.depth_bound(*n)
        worst = rs.ratio_to_bound(got, rs.exact(fields, centre, DELTA, nbins, PAIRS, RADIALS),
                                  rs.abs_sums(fields, centre, DELTA, nbins, PAIRS, RADIALS), bound)
        print(n, which, nbins, "worst |twin - exact| / (depth_bound sum |term|) = %.3g, depth_bound = %.3g" % (worst, bound))
        assert worst <= 1.0, (n, which, nbins, worst)
        # coverage: every site is in a shell when nbins * delta covers the half diagonal, fewer with a short nbins
        if which == "nan":
            assert not counts.any() and not sums.any() and not np.signbit(sums).any()      # all counts 0, all sums +0.0
        elif nbins == 3:
            assert 0 < counts.sum() < nsites
        else:
            assert nbins * DELTA > 0.5 * math.sqrt(sum(v * v for v in n)) and counts.sum() == nsites


def test_the_centre_site_and_the_ties_of_the_minimum_image(pkg):
    """An integer centre: shell 0 of width 1/2 holds the centre site alone, whose radial terms are +0.0 and whose other
    terms are the site's own.  On an even axis the site at d = +n/2 is taken to -n/2: its projection changes sign."""
    n = (32, 16, 3)
    fields = _random_fields(n)
    cx, cy, cz = (int(v) for v in rs.centres(n)["integer"])
    counts, sums = pkg.analysis.radial_shells(fields, (cx, cy, cz), 0.5, 4, PAIRS, RADIALS)
    x = fields[:, cz, cy, cx]
    assert counts[0] == 1.0
    assert np.array_equal(sums[:6, 0], [x[0], x[1], x[2], x[0] * x[1], x[2] * x[2], x[1] * x[0]])
    assert np.array_equal(sums[6:, 0], [0.0, 0.0]) and not np.signbit(sums[6:, 0]).any()
    # the tie on y: iy = cy + 8 is at d = +8 = n/2, taken to -8; with x and z on the centre, r = 8 and v . r^ = -v_y
    one = np.zeros((3, 3, 16, 32))
    one[:, cz, cy + 8, cx] = (2.0, 3.0, 5.0)
    _, s = pkg.analysis.radial_shells(one, (cx, cy, cz), 1.0, 9, (), [(None, (0, 1, 2))])
    assert s[3, 8] == -3.0 and np.count_nonzero(s[3]) == 1
    # the tie on x: ix = cx - 16 is at d = -16 = -n/2, which stays
    one[:] = 0.0
    one[:, cz, cy, cx - 16] = (2.0, 3.0, 5.0)
    _, s = pkg.analysis.radial_shells(one, (cx, cy, cz), 1.0, 17, (), [(None, (0, 1, 2))])
    assert s[3, 16] == -2.0 and np.count_nonzero(s[3]) == 1


def test_radial_shells_refuses_bad_arguments(pkg):
    f = np.zeros((2, 3, 4, 5))
    an = pkg.analysis
    for bad in (lambda: an.radial_shells(f, (1, 1, 1), 1.0, 4, [(0, 2)]), lambda: an.radial_shells(f, (1, 1, 1), 1.0, 4, (), [(2, (0, 1, 1))]),
                lambda: an.radial_shells(f, (1, 1, 1), 1.0, 4, (), [(None, (0, 1))]), lambda: an.radial_shells(f, (1, 1, 1), 0.0, 4),
                lambda: an.radial_shells(f, (1, 1, 1), 1.0, 129), lambda: an.radial_shells(f, (1, 1), 1.0, 4),
                lambda: an.radial_shells(f[0], (1, 1, 1), 1.0, 4)):
        with pytest.raises(ValueError):
            bad()
    counts, sums = an.radial_shells(f, (1, 1, 1), 1.0, 4)
    assert counts.shape == (4,) and sums.shape == (2, 4)


# ---- a tanh droplet made by hand -------------------------------------------------------------------------------------------
HI_R, LO_R, HI_P, LO_P, R0, W0, ALPHA0, CS2 = 3.4, 0.02, -0.003, 3.05, 8.0, 1.0, 1.5, 1.0 / 3.0


def _tanh_droplet(n=32, centre=(15.3, 16.1, 15.7)):
    """rho inside HI_R, outside LO_R, phi inside HI_P, outside LO_P, both tanh profiles of radius R0 and width W0 about a
    centre on no lattice site; af = -cs2 alpha0 grad phi and ag = -cs2 alpha0 grad rho analytically (radial vectors)."""
    i = np.arange(n, dtype=np.float64)
    d = [np.where(i - c >= n / 2, i - c - n, np.where(i - c < -n / 2, i - c + n, i - c)) for c in centre]
    dx, dy, dz = d[0][None, None, :], d[1][None, :, None], d[2][:, None, None]
    r = np.sqrt((dx * dx + dy * dy) + dz * dz)
    t = np.tanh((r - R0) / W0)
    rho, phi = HI_R - (HI_R - LO_R) / 2 * (1 + t), HI_P - (HI_P - LO_P) / 2 * (1 + t)
    drho, dphi = -(HI_R - LO_R) / 2 * (1 - t * t) / W0, -(HI_P - LO_P) / 2 * (1 - t * t) / W0
    unit = [np.broadcast_to(v, r.shape) / r for v in (dx, dy, dz)]
    af = [-CS2 * ALPHA0 * dphi * u for u in unit]
    ag = [-CS2 * ALPHA0 * drho * u for u in unit]
    return np.array([rho, phi] + af + ag), centre, r, (drho, dphi)


def test_pair_and_radial_terms_and_the_laplace_helpers_on_a_tanh_droplet(pkg):
    """The pair and radial sums against direct numpy expressions over the shells' masks; radial_pressure and pressure_jump
    against the constructed plateaus: |tanh - +-1| <= 2 e^{-2 x} bounds what the plateaus miss at x = |r - R0| / W0 widths
    from the interface, and p is bilinear in (rho, phi); fit_radial_profile against R0 and W0: the profile is monotonic, so
    a shell's mean lies between the profile's values at the shell's two edges: the fitted data are the true profile read
    at radii displaced by at most delta / 2, which moves the midpoint by at most delta / 2 and the half width of the
    transition by at most delta / 2."""
    an = pkg.analysis
    fields, centre, r, (drho, dphi) = _tanh_droplet()
    names, pairs, radials = an.laplace_inputs()
    assert names == "rho phi afx afy afz agx agy agz".split() and pairs == [("rho", "phi")]
    assert radials == [("rho", ("afx", "afy", "afz")), ("phi", ("agx", "agy", "agz"))]
    ps = [(names.index(a), names.index(b)) for a, b in pairs]
    rd = [(names.index(w), tuple(names.index(c) for c in v)) for w, v in radials]
    delta = 0.5
    nbins = rs.default_bins((32, 32, 32), delta)
    counts, sums = an.radial_shells(fields, centre, delta, nbins, ps, rd)
    assert counts.sum() == 32 ** 3 and sums.shape == (11, nbins)
    shell = np.floor(r / delta).astype(int)
    rho, phi = fields[0], fields[1]
    direct = {8: rho * phi, 9: rho * (-CS2 * ALPHA0 * dphi), 10: phi * (-CS2 * ALPHA0 * drho)}       # v . r^ of a radial vector g r^ is g
    for q, term in direct.items():
        want = np.array([term[shell == k].sum() for k in range(nbins)])
        scale = np.array([np.abs(term[shell == k]).sum() for k in range(nbins)])
        assert np.all(np.abs(sums[q] - want) <= 1e-12 * scale), q
    assert np.array_equal(counts, np.bincount(shell.ravel(), minlength=nbins))
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.where(counts > 0, sums / counts, np.nan)
    rr = (np.arange(nbins) + 0.5) * delta
    p = an.radial_pressure(means, names, ALPHA0, CS2)
    r_in, r_out = 2.0, 14.0

    def missed(x):                                         # what p misses of a plateau (rho_0, phi_0) x widths away
        er, ep = (HI_R - LO_R) * math.exp(-2 * x), abs(HI_P - LO_P) * math.exp(-2 * x)
        return lambda rho_0, phi_0: CS2 * (er + ep) + ALPHA0 * CS2 * (abs(rho_0) * ep + abs(phi_0) * er + er * ep)
    p_in, p_out = CS2 * (HI_R + HI_P) + ALPHA0 * CS2 * HI_R * HI_P, CS2 * (LO_R + LO_P) + ALPHA0 * CS2 * LO_R * LO_P
    tol = missed((R0 - r_in) / W0)(HI_R, HI_P) + missed((r_out - R0) / W0)(LO_R, LO_P) + 1e-13
    dp = an.pressure_jump(p, counts, rr, r_in, r_out)
    print("Delta p %.12g, constructed %.12g, difference %.3g, tolerance %.3g" % (dp, p_in - p_out, dp - (p_in - p_out), tol))
    assert tol < 2e-3 * abs(p_in - p_out) and abs(dp - (p_in - p_out)) <= tol
    assert np.isnan(an.pressure_jump(p, counts, rr, 0.0, r_out))                               # no shell inside
    hi, lo, R, W = an.fit_radial_profile(rr, means[0], counts)
    print("fit: hi %.6f lo %.6f R %.6f W %.6f (constructed %.1f %.2f %.1f %.1f), delta / 2 = %.2f" % (hi, lo, R, W, HI_R, LO_R, R0, W0, delta / 2))
    assert abs(R - R0) <= delta / 2 and abs(W - W0) <= delta / 2
    # the equimolar radius, in cells: the integral of r^2 times the Fermi function 1/2 (1 - tanh((r - R0) / W0)) gives
    # R_e^3 = R0^3 + (pi W0 / 2)^2 R0, here R_e = 8.1015: inside one shell width of R0, as for any W0 << R0
    Re = an.equimolar_radius(means[0], counts)
    print("equimolar radius %.6f, continuum %.6f" % (Re, (R0 ** 3 + (math.pi * W0 / 2) ** 2 * R0) ** (1 / 3)))
    assert abs(Re - R0) <= delta
    # the force integral: -(sum over the shells below n / 2 of <rho af . r^> + <phi ag . r^>) delta / n, positive for this droplet
    f = an.radial_force_integral(means, names, delta, 32)
    inside = rr < 16.0
    assert f == -(np.where(inside, means[9] + means[10], 0.0).sum()) * delta / 32 and f > 0
    # leading axes [count, B] pass through
    stacked = np.broadcast_to(means, (2, 3) + means.shape)
    assert np.array_equal(an.radial_pressure(stacked, names, ALPHA0, CS2)[1, 2], p, equal_nan=True)     # the last shell is empty
    assert np.array_equal(an.pressure_jump(an.radial_pressure(stacked, names, ALPHA0, CS2), np.broadcast_to(counts, (2, 3, nbins)), rr, r_in, r_out),
                          np.full((2, 3), dp))
    with pytest.raises(ValueError, match="Q = 8 variables"):
        an.radial_pressure(means[:10], names, ALPHA0, CS2)
    with pytest.raises(ValueError, match="'rho' is missing"):
        an.radial_pressure(means, ["x"] + names[1:], ALPHA0, CS2)


# ---- the four golden droplets --------------------------------------------------------------------------------------------------
def _notebook_dp(rec):
    """p_in - p_out of a notebook record: ideal-gas Delta P minus the printed interaction difference (out minus in)."""
    return rec[6] - rec[7]


def test_golden_droplets_give_the_laplace_law(pkg):
    """From tests/golden/radial_droplets.npz alone (the CPU oracle's records, make_golden_radial.py): Delta p of the shell
    means (inside r < 3, outside r >= 16 cells), the radius of the 1-D tanh fit and the two-point Laplace slope / 2
    against what Surface_Tension.ipynb records from single lattice lines and 3-D fits (CELL13 / CELL18, R_15 / R_17,
    GAMMA_15[2] / GAMMA_17[2]).  Measured on the golden, shell value / notebook value:
        system          Delta p    R
        a15_k01_r20     1.0033     1.0001
        a15_k01_r30     0.9991     1.0025
        a17_k10_r20     1.0005     1.0019
        a17_k10_r28     0.9997     1.0017
        slope / 2:      a15_k01 1.0060, a17_k10 1.0048
    The bands are these ratios widened to the next 0.01 on either side: Delta p in [0.99, 1.01], R in [1.00, 1.01],
    slope / 2 in [1.00, 1.01].  A wrong sign puts a ratio at -1, a factor 2 at 2 or 0.5; a missing 1 / counts multiplies
    every shell by its site count (thousands outside, a handful inside), which takes Delta p and the fit far from 1.  The
    minimum image is NOT seen by this test: the droplets sit at (16, 16, 16) of a 32-cell box, where i - c lies in
    [-16, 16) already; the corner centres of the definition tests above are what hold it."""
    golden = {k.replace("__", "/"): v for k, v in np.load(GOLDEN).items()}
    an = pkg.analysis
    names, _, _ = an.laplace_inputs()
    nbins = int(golden["nbins"])
    n = tuple(int(v) for v in golden["shape"])
    cs2 = 1.0 / 3.0
    r = (np.arange(nbins) + 0.5) * 1.0
    notebook = {"a15_k01_r20": (1.5, CELL13[0], R_15[0]), "a15_k01_r30": (1.5, CELL13[4], R_15[4]),
                "a17_k10_r20": (1.7, CELL18[0], R_17[0]), "a17_k10_r28": (1.7, CELL18[3], R_17[3])}
    found = {}
    for case, (alpha0, cell, R_nb) in notebook.items():
        rec = golden["rec/" + case]
        assert rec.shape == (3 + 12 * nbins,) and np.array_equal(rec[:3], golden["centre/" + case])
        counts, sums = rec[3:3 + nbins], rec[3 + nbins:].reshape(11, nbins)
        assert counts.sum() == n[0] * n[1] * n[2]
        with np.errstate(invalid="ignore", divide="ignore"):
            means = np.where(counts > 0, sums / counts, np.nan)
        dp = float(an.pressure_jump(an.radial_pressure(means, names, alpha0, cs2), counts, r, 3.0, 16.0))
        R = an.fit_radial_profile(r, means[0], counts)[2] / n[0]
        force = float(an.radial_force_integral(means, names, 1.0, n[0]))
        assert dp == float(golden["dp/" + case]) and force == float(golden["force/" + case])
        assert abs(R - float(golden["R/" + case])) <= 1e-9 * R                                 # an iterative fit: not bit for bit
        print("%s: Delta p %.12g (notebook %.12g, ratio %.4f), R %.9f (notebook %.8f, ratio %.4f), force integral %.6g (notebook's line %.6g)"
              % (case, dp, _notebook_dp(cell), dp / _notebook_dp(cell), R, R_nb, R / R_nb, force, cell[5]))
        assert 0.99 <= dp / _notebook_dp(cell) <= 1.01, (case, dp / _notebook_dp(cell))
        assert 1.00 <= R / R_nb <= 1.01, (case, R / R_nb)
        assert force > 0
        found[case] = (dp, float(golden["R/" + case]))
    for pset, a, b, gamma in (("a15_k01", "a15_k01_r20", "a15_k01_r30", GAMMA_15[2]), ("a17_k10", "a17_k10_r20", "a17_k10_r28", GAMMA_17[2])):
        half_slope = (found[a][0] - found[b][0]) / (1.0 / found[a][1] - 1.0 / found[b][1]) / 2.0
        assert half_slope == float(golden["gamma/" + pset])
        print("%s: two-point Laplace slope / 2 = %.12g (notebook's regression %.12g, ratio %.4f)" % (pset, half_slope, gamma, half_slope / gamma))
        assert 1.00 <= half_slope / gamma <= 1.01, (pset, half_slope / gamma)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
_C_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}


def _declared_arguments(header, name):
    """The ctypes argument list the declaration of `name` in include/bflbm.h asks for: handles and double buffers are
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


def test_radial_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in RADIAL_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_radial_create"] == sig["bflbm_batch_radial_create"]
    # (owner, source, nvars, vars, npairs, pair_a, pair_b, nrad, rad_w, rad_v, centre, threshold, delta, nbins, every, capacity, out)
    assert len(sig["bflbm_radial_create"][1]) == 17 and sig["bflbm_radial_create"][1][15] is ctypes.c_longlong
    assert header.count("Radial traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert hasattr(pkg, "RadialTrace") and "RadialTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "radial_trace")
    assert not hasattr(pkg.RingLBM, "radial_trace")        # rings of z-slabs are out of scope
    for fn in ("radial_shells", "laplace_inputs", "radial_pressure", "pressure_jump", "radial_force_integral", "fit_radial_profile",
               "equimolar_radius"):
        assert hasattr(pkg.analysis, fn)
    # the header, the numpy twin and the tests' emulation state the same constants
    assert (pkg.analysis.RADIAL_TILE, pkg.analysis.RADIAL_MAX_BINS) == (rs.TILE, rs.MAX_BINS) == (256, 128)
    block = header[header.index("Radial traces:"):header.index("typedef struct bflbm_radial")]
    assert "tiles of 256 consecutive sites" in block and "nbins in 1..128" in block


def test_radial_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_double * 8)()
    va, pa = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(0)
    rv = (ctypes.c_int * 3)(0, 0, 0)
    g = [ctypes.c_int() for _ in range(4)]

    def create(fn, owner=None, variables=va, out=ctypes.byref(h)):
        return getattr(lib, fn)(owner, 0, 1, variables, 1, pa, pa, 1, pa, rv, None, 0.06, 1.0, 4, 1, 4, out)
    calls = {
        "bflbm_radial_create": lambda: create("bflbm_radial_create"),
        "bflbm_batch_radial_create": lambda: create("bflbm_batch_radial_create"),
        "bflbm_radial_sample": lambda: lib.bflbm_radial_sample(None),
        "bflbm_radial_reset": lambda: lib.bflbm_radial_reset(None),
        "bflbm_radial_count": lambda: lib.bflbm_radial_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_radial_geometry": lambda: lib.bflbm_radial_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_radial_read": lambda: lib.bflbm_radial_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a handle that is not null but no variables, or no place for the result: refused before the handle is read
    fake = ctypes.c_void_p(8)
    for fn in ("bflbm_radial_create", "bflbm_batch_radial_create"):
        assert create(fn, owner=fake, variables=None) != 0 and "null" in lib.bflbm_last_error().decode()
        assert create(fn, owner=fake, out=None) != 0 and fn in lib.bflbm_last_error().decode()
    assert lib.bflbm_radial_destroy(None) == 0              # like every destroy of the ABI: nothing to do


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_radial_kernel_metadata(device_asm):
    """k_radial_shells<NV>, NV = 1 .. 8, and k_radial_finish: no scratch; the shell kernel's LDS is the 2048 (NV + 4) + 1312
    bytes include/bflbm.h states (six workgroups of the largest fit the 160 KiB of a compute unit), the finishing kernel
    uses none."""
    found = kernels(device_asm, r"^_Z\w*?15k_radial_shellsILi(\d)EE\w*:")        # Itanium mangling: <length><name>
    assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9))
    for m, meta in found:
        lds = 2048 * (int(m.group(1)) + 4) + 1312
        assert re.search(r"; LDSByteSize: %d\b" % lds, meta), f"{m.group(0)}: LDS"
        assert 6 * lds <= 160 * 1024
    finish = kernels(device_asm, r"^_Z\w*?15k_radial_finish(E)\w*:")
    assert len(finish) == 1 and re.search(r"; LDSByteSize: 0\b", finish[0][1])
    for m, meta in found + finish:
        assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
