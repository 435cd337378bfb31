"""Shape traces, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must fail before
any device is touched), analysis.droplet_radii against a plain loop, the quadrature and harmonics of analysis.ray_nodes /
real_harmonics, planted shape modes of an analytic droplet, and the compiled kernels (hipcc cross-compiles gfx950, no GPU
needed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernel_of, mangled   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE_SYMBOLS = ["bflbm_shape_create", "bflbm_batch_shape_create", "bflbm_shape_destroy", "bflbm_shape_sample",
                 "bflbm_shape_reset", "bflbm_shape_count", "bflbm_shape_geometry", "bflbm_shape_read"]


def test_shape_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in SHAPE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert hasattr(pkg, "ShapeTrace") and "ShapeTrace" in pkg.__all__
    assert hasattr(pkg.BinaryLBM, "shape_trace") and hasattr(pkg.BatchLBM, "shape_trace")


def test_shape_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    g = [ctypes.c_int() for _ in range(4)]
    buf = (ctypes.c_double * 8)()
    u = (ctypes.c_double * 3)(0.0, 0.0, 1.0)
    calls = {
        "bflbm_shape_create": lambda: lib.bflbm_shape_create(None, 0, 0.5, 0, None, 0.06, 1, u, 0.5, 8, 1, 4, ctypes.byref(h)),
        "bflbm_batch_shape_create": lambda: lib.bflbm_batch_shape_create(None, 0, 0.5, 0, None, 0.06, 1, u, 0.5, 8, 1, 4, ctypes.byref(h)),
        "bflbm_shape_sample": lambda: lib.bflbm_shape_sample(None),
        "bflbm_shape_reset": lambda: lib.bflbm_shape_reset(None),
        "bflbm_shape_count": lambda: lib.bflbm_shape_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_shape_geometry": lambda: lib.bflbm_shape_geometry(None, *[ctypes.byref(v) for v in g]),
        "bflbm_shape_read": lambda: lib.bflbm_shape_read(None, 0, 1, buf, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_shape_destroy(None) == 0            # like every destroy of the ABI: nothing to do


# ---- analysis.droplet_radii against a plain loop ---------------------------------------------------------------------------
def _radii_loop(d, centre, dirs, level, step, nsteps, rising):
    """The definition of include/bflbm.h, one ray and one k at a time, in Python floats (IEEE doubles)."""
    nz, ny, nx = d.shape

    def density(p):
        if not all(abs(v) < 2.0 ** 30 for v in p):         # false for a NaN
            return math.nan
        i = [math.floor(v) for v in p]
        f = [v - float(k) for v, k in zip(p, i)]
        x0, y0, z0 = i[0] % nx, i[1] % ny, i[2] % nz        # Python's % wraps negatives into [0, n)
        x1, y1, z1 = (i[0] + 1) % nx, (i[1] + 1) % ny, (i[2] + 1) % nz
        c = {}
        for (b, yy) in ((0, y0), (1, y1)):
            for (a, zz) in ((0, z0), (1, z1)):
                lo, hi = float(d[zz, yy, x0]), float(d[zz, yy, x1])
                c[(b, a)] = lo + f[0] * (hi - lo)
        c0 = c[(0, 0)] + f[1] * (c[(1, 0)] - c[(0, 0)])
        c1 = c[(0, 1)] + f[1] * (c[(1, 1)] - c[(0, 1)])
        return c0 + f[2] * (c1 - c0)

    out = np.full(len(dirs), np.nan)
    for j, u in enumerate(dirs):
        u = [float(v) for v in u]
        prev = density([float(centre[a]) + (0.0 * step) * u[a] for a in range(3)])
        for k in range(1, nsteps + 1):
            t = float(k) * step
            cur = density([float(centre[a]) + t * u[a] for a in range(3)])
            if rising:
                hit = prev < level <= cur
            else:
                hit = prev >= level > cur
            if hit:
                frac = (level - prev) / (cur - prev) if rising else (prev - level) / (prev - cur)
                out[j] = step * (float(k - 1) + frac)
                break
            prev = cur
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_droplet_radii_against_a_plain_loop(pkg):
    rng = np.random.default_rng(7)
    nz, ny, nx = 13, 5, 7
    d = 0.5 + 0.3 * rng.standard_normal((nz, ny, nx))                 # many crossings per ray, both ways
    dirs = pkg.analysis.ray_nodes(4, 8)[0]
    dirs = np.concatenate([dirs, np.eye(3), -np.eye(3)])               # the axes: sample points on lattice sites
    seen_nan = seen_finite = False
    for centre in ((3.3, 2.1, 6.7), (0.2, 0.4, 0.1), (3.0, 2.0, 6.0), (-4.5, -7.25, -20.5), (6.9, 4.9, 12.9)):
        for step, nsteps in ((0.5, 9), (0.37, 30), (1.0, 3), (2.5, 1)):
            for direction, rising in (("falling", 0), ("rising", 1)):
                got = pkg.analysis.droplet_radii(d, centre, dirs, 0.5, step, nsteps, direction)
                want = _radii_loop(d, centre, dirs, 0.5, step, nsteps, rising)
                assert got.shape == (len(dirs),) and _same(got, want), (centre, step, nsteps, direction)
                assert _same(got, pkg.analysis.droplet_radii(d, centre, dirs, 0.5, step, nsteps, rising))
                seen_nan |= bool(np.isnan(got).any())
                seen_finite |= bool(np.isfinite(got).any())
    assert seen_nan and seen_finite
    # the low-side centres above make rays leave the box downward: floor of a negative coordinate, wrapped
    low = pkg.analysis.droplet_radii(d, (0.2, 0.4, 0.1), -np.eye(3), 0.5, 0.5, 9)
    assert _same(low, _radii_loop(d, (0.2, 0.4, 0.1), -np.eye(3), 0.5, 0.5, 9, 0)) and np.isfinite(low).any()
    with pytest.raises(ValueError):
        pkg.analysis.droplet_radii(d[0], (0, 0, 0), dirs, 0.5, 0.5, 4)
    with pytest.raises(ValueError):
        pkg.analysis.droplet_radii(d, (0, 0, 0), dirs, 0.5, 0.5, 4, "sideways")
    with pytest.raises(ValueError):
        pkg.analysis.droplet_radii(d, (0, 0, 0), dirs, 0.5, 0.0, 4)
    with pytest.raises(ValueError):
        pkg.analysis.droplet_radii(d, (0, 0, 0), dirs, 0.5, 0.5, 0)


def test_droplet_radii_edge_cases(pkg):
    level = 0.5
    ez = np.array([[0.0, 0.0, 1.0]])
    radii = pkg.analysis.droplet_radii

    def field(col):
        return np.asarray(col, dtype=np.float64)[:, None, None].repeat(2, axis=1).repeat(3, axis=2)

    # a value exactly at the level: as d_k it closes a rising pair, as d_{k-1} it opens a falling pair (step 1 from a
    # site: the sample points are the sites of the column)
    col = [0.2, 0.5, 0.9, 0.5, 0.1, 0.5, 0.5, 0.7]
    d = field(col)
    for rising, want in ((1, 1.0), (0, 3.0)):
        got = radii(d, (1.0, 0.0, 0.0), ez, level, 1.0, 7, rising)
        assert _same(got, _radii_loop(d, (1.0, 0.0, 0.0), ez, level, 1.0, 7, rising)) and got[0] == want
    # from z = 4 upward: 0.1 -> 0.5 rises on the first pair (r = 1 exactly); the pair (0.5, 0.5) is flat: no crossing either
    # way; 0.5 -> 0.7 does not rise (d_{k-1} < level fails), and nothing falls before the wrap
    assert radii(d, (1.0, 0.0, 4.0), ez, level, 1.0, 3, 1)[0] == 1.0
    assert np.isnan(radii(d, (1.0, 0.0, 5.0), ez, level, 1.0, 2, 1)[0]) and np.isnan(radii(d, (1.0, 0.0, 5.0), ez, level, 1.0, 2, 0)[0])
    flat = np.full((4, 2, 2), level)
    for rising in (0, 1):
        assert np.isnan(radii(flat, (0.3, 0.2, 0.1), pkg.analysis.ray_nodes(2, 4)[0], level, 0.5, 12, rising)).all()
    # a NaN site satisfies neither condition: the crossing through it is lost, the next one is found
    e = field([0.2, np.nan, 0.9, 0.1, 0.8, 0.3])
    for rising in (0, 1):
        got = radii(e, (0.0, 1.0, 0.0), ez, level, 1.0, 5, rising)
        assert _same(got, _radii_loop(e, (0.0, 1.0, 0.0), ez, level, 1.0, 5, rising))
    assert radii(e, (0.0, 1.0, 0.0), ez, level, 1.0, 5, 0)[0] == 1.0 * (2.0 + (0.9 - 0.5) / (0.9 - 0.1))
    assert radii(e, (0.0, 1.0, 0.0), ez, level, 1.0, 5, 1)[0] == 1.0 * (3.0 + (0.5 - 0.1) / (0.8 - 0.1))
    # a level never reached
    dirs = pkg.analysis.ray_nodes(3, 6)[0]
    for lv in (2.0, -1.0):
        for rising in (0, 1):
            assert np.isnan(radii(d, (1.2, 0.7, 3.1), dirs, lv, 0.5, 20, rising)).all()
    # a NaN centre, and one too far out to index: every radius NaN, as in the loop
    for centre in ((np.nan, 0.5, 3.0), (1.0, np.inf, 3.0), (1.0, 0.5, 2.0 ** 31)):
        got = radii(d, centre, dirs, level, 0.5, 20)
        assert np.isnan(got).all() and _same(got, _radii_loop(d, centre, dirs, level, 0.5, 20, 0))


# ---- the quadrature and the harmonics ---------------------------------------------------------------------------------------
def test_ray_nodes_integrate_the_harmonics_exactly(pkg):
    """The Gauss-Legendre x equispaced product rule with 16 x 32 nodes is exact for products of two harmonics of l <= 4
    (degree 8 < 32), and 512 terms of size <= 1 round far below 1e-13."""
    eps = np.finfo(np.float64).eps
    for nt, nph in ((16, 32), (4, 8), (5, 3)):
        dirs, w = pkg.analysis.ray_nodes(nt, nph)
        assert dirs.shape == (nt * nph, 3) and w.shape == (nt * nph,)
        assert abs(w.sum() - 4 * math.pi) <= 8 * eps * 4 * math.pi        # 8 eps relative: the sum of the weights itself rounds
        assert abs(math.fsum(w) - 4 * math.pi) <= 8 * eps * 4 * math.pi
        assert np.abs((dirs * dirs).sum(axis=1) - 1.0).max() <= 8 * eps
    dirs, w = pkg.analysis.ray_nodes(16, 32)
    assert np.array_equal(dirs[0, 2], dirs[31, 2]) and dirs[0, 2] != dirs[32, 2]     # theta-major
    assert dirs[0, 1] > 0 and abs(dirs[0, 1] / dirs[0, 0] - math.tan(math.pi / 32)) < 1e-12   # phi offset by half a cell
    Y = pkg.analysis.real_harmonics(dirs, 4)
    assert Y.shape == (512, 25)
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(25)).max() <= 1e-13
    # the first few against their closed forms
    x, y, z = dirs.T
    for idx, f in ((0, np.full(512, 0.5 / math.sqrt(math.pi))), (1, math.sqrt(3 / (4 * math.pi)) * y),
                   (2, math.sqrt(3 / (4 * math.pi)) * z), (3, math.sqrt(3 / (4 * math.pi)) * x),
                   (6, math.sqrt(5 / (16 * math.pi)) * (3 * z * z - 1)), (8, math.sqrt(15 / (16 * math.pi)) * (x * x - y * y)),
                   (4, math.sqrt(15 / (4 * math.pi)) * x * y)):
        assert np.abs(Y[:, idx] - f).max() < 1e-14, idx
    with pytest.raises(ValueError):
        pkg.analysis.ray_nodes(0, 4)
    with pytest.raises(ValueError):
        pkg.analysis.real_harmonics(dirs[:, :2], 2)


# ---- planted modes on an analytic droplet -----------------------------------------------------------------------------------
R0, WIDTH, CENTRE, N = 8.3, 1.5, (15.3, 16.1, 15.7), 32
PLANTED = {(2, 0): 0.03, (2, 2): -0.02, (3, 1): 0.015}


def _analytic_droplet(pkg, planted):
    z, y, x = np.meshgrid(np.arange(N) - CENTRE[2], np.arange(N) - CENTRE[1], np.arange(N) - CENTRE[0], indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    u = np.stack([x / r, y / r, z / r], axis=-1).reshape(-1, 3)          # no lattice site is the centre
    Y = pkg.analysis.real_harmonics(u, 4)
    R = np.full(len(u), 1.0)
    for (l, m), a in planted.items():
        R = R + a * Y[:, l * l + l + m]
    return 0.5 * (1.0 - np.tanh((r - R0 * R.reshape(r.shape)) / WIDTH))


def _modes_of(pkg, rho):
    dirs, w = pkg.analysis.ray_nodes(16, 32)
    r = pkg.analysis.droplet_radii(rho, CENTRE, dirs, 0.5, 0.5, 32)
    assert np.isfinite(r).all()
    return pkg.analysis.shape_modes(r, dirs, w, 4), r, dirs, w


def test_planted_modes_are_recovered(pkg):
    """rho = (1 - tanh((r - R(u)) / 1.5)) / 2 in 32^3 with R(u) = 8.3 (1 + 0.03 Y_20 - 0.02 Y_22 + 0.015 Y_31) about
    (15.3, 16.1, 15.7), level 0.5, step 0.5, ray_nodes(16, 32).  Bounds (set with the feature, not from these numbers):
    every l = 1 ... 4 coefficient within 3e-3 x 8.3 = 0.0249 of the planted one, a tenth of the largest planted mode; the
    unperturbed sphere keeps every l >= 1 mode below 0.015 lattice units, the thermal rms of an l = 2 mode at kBT = 1e-5,
    gamma = 0.0108.  Measured: planted droplet, largest deviation 0.00735 lattice units = 8.9e-4 x 8.3; sphere, largest l >= 1 mode 0.00487
    (the (1, 0) coefficient: the centre is off the lattice sites), a_00 / sqrt(4 pi) = 8.279."""
    a, r, dirs, w = _modes_of(pkg, _analytic_droplet(pkg, PLANTED))
    assert a.shape == (25,)
    worst = 0.0
    for l in range(1, 5):
        for m in range(-l, l + 1):
            want = R0 * PLANTED.get((l, m), 0.0)
            dev = abs(a[l * l + l + m] - want)
            worst = max(worst, dev)
            assert dev <= 3e-3 * R0, (l, m, a[l * l + l + m], want)
    print("planted: largest deviation", worst, worst / R0)
    assert abs(a[0] / math.sqrt(4 * math.pi) - R0) < 0.05             # the mean radius, for orientation only

    a0, r0, _, _ = _modes_of(pkg, _analytic_droplet(pkg, {}))
    print("sphere: largest l >= 1 mode", np.abs(a0[1:]).max(), int(np.abs(a0[1:]).argmax()) + 1, "mean radius", a0[0] / math.sqrt(4 * math.pi))
    assert np.abs(a0[1:]).max() < 0.015

    # shape_modes is the weighted sum it says it is; leading axes pass through and a NaN stays in its own frame
    Y = pkg.analysis.real_harmonics(dirs, 4)
    direct = np.array([sum(w[j] * r[j] * Y[j, k] for j in range(len(w))) for k in range(25)])
    assert np.abs(direct - a).max() <= 512 * np.finfo(np.float64).eps * np.abs(w * r).sum()
    frames = np.stack([r, r0, r])
    frames[2, 17] = np.nan
    both = pkg.analysis.shape_modes(frames.reshape(3, 1, -1), dirs, w, 4)
    assert both.shape == (3, 1, 25) and np.array_equal(both[0, 0], a) and np.array_equal(both[1, 0], a0) and np.isnan(both[2]).all()
    with pytest.raises(ValueError):
        pkg.analysis.shape_modes(r[:-1], dirs, w, 4)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k_shape_density", "k_shape_density_batch", "k_shape_rays", "k_shape_finish"])
def test_shape_kernel_compiled_without_scratch(device_asm, kernel):
    _, meta = kernel_of(device_asm, mangled(kernel), "shape kernel")
    assert re.search(r"; ScratchSize: 0\b", meta), f"{kernel} spills to scratch"
