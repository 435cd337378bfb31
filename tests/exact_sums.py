"""Exact references and a-priori bounds for the device-side sums of rho (csrc/bflbm_droplet.h, bflbm_trace.h, k_reduce).

exact_moments adds the terms of the raw moments {1, x, y, z, xx, xy, xz, yy, yz, zz} of a density field in integer
arithmetic: a double is an integer mantissa times a power of two, the monomials are integers, so the sum of the exact
products is an integer over a power of two and the reference has no rounding at all.  depth_bound is the relative error
a sum of the device may have against it, from the number of roundings a term passes through in the order the kernels add
(the summation order is fixed and documented there), so the tests that use the pair need no measured tolerance.

emulate_two_stage restates that order in numpy (tests/test_exact_sums.py holds it against the bound on the CPU).
No GPU is needed for anything here."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                     # unit roundoff of a double
BLOCK = 256                        # sites per stage-1 block, threads of stage 2
MONOMIALS = ((), (0,), (1,), (2,), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # axes 0, 1, 2 = x, y, z


def pitch_of(nx):
    """Row stride of the resident planes (domain_geo in csrc/bflbm.hip)."""
    return (nx + 15) & ~15 if nx > 16 else nx


def blocks_per_plane(nx, ny):
    return (pitch_of(nx) * ny + BLOCK - 1) // BLOCK


def depth_bound(kind, nx, ny, nz, nslabs=1):
    """d u / (1 - d u): the relative error, against sum |term|, of a sum whose every term passes through at most d
    roundings (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, for any fixed order).
    "two_stage" (droplet moments, traces; the same for a ring, whose planes are added in the lone order):
        d = 1 (the product rho * monomial) + 8 (tree of block_reduce) + ceil(nbx / 256) (the strided pass of stage 2)
            + 8 (its tree) + nz (the planes in sequence)
    "host_blocks" (mass, com_sums: reduce5 adds the nbx * nz block sums of a slab in sequence on the host; a ring adds
    its slabs' sums after that):
        d = 1 + 8 + nbx * (planes of the largest slab) [+ nslabs for a ring]"""
    nbx = blocks_per_plane(nx, ny)
    if kind == "two_stage":
        d = 1 + 8 + -(-nbx // BLOCK) + 8 + nz
    elif kind == "host_blocks":
        d = 1 + 8 + nbx * -(-nz // nslabs) + (nslabs if nslabs > 1 else 0)
    else:
        raise ValueError(f"depth_bound: unknown kind {kind!r}")
    return d * U / (1 - d * U)


def _mantissas(a):
    """a == m * 2.0 ** e with int64 m, |m| < 2^53, and int64 e, element by element."""
    m, e = np.frexp(a)
    m = np.ldexp(m, 53)
    mi = m.astype(np.int64)
    assert np.array_equal(mi.astype(np.float64), m)
    return mi, e.astype(np.int64) - 53


def _exact_dot(mant, expo, weights):
    """[sum_i mant_i 2^(expo_i - emin) w_i for w in weights], emin: Python ints.  mant int64 (|.| < 2^53), w int64 >= 0.
    The mantissas go in 16-bit limbs, so that a chunk of products adds up inside an int64."""
    emin = int(expo.min()) if expo.size else 0
    sign = np.sign(mant)
    mag = np.abs(mant)
    limbs = [(mag >> (16 * k)) & 0xFFFF for k in range(4)]
    groups = [(int(e), expo == e) for e in np.unique(expo)]
    out = []
    for w in weights:
        wmax = int(w.max()) if w.size else 0
        chunk = max(1, (1 << 62) // (0xFFFF * max(wmax, 1)))          # products of one chunk stay below 2^62
        sw = sign * w
        total = 0
        for e, sel in groups:
            swe = np.where(sel, sw, 0)
            for k, limb in enumerate(limbs):
                t = limb * swe
                s = sum(int(t[i:i + chunk].sum()) for i in range(0, t.size, chunk))
                total += s << (16 * k + e - emin)
        out.append(total)
    return out, emin


def exact_moments(rho_zyx, weighted=False, threshold=None):
    """(moments, abs_sums): lists of Fractions, the exact sums of rho * monomial (global cell indices) over the lattice
    rho_zyx[nz, ny, nx] and of |rho * monomial|.
    weighted: the trapezoid-weighted set of k_moments, the first and the last plane of every direction counted half (a
    direction of one plane is halved once).
    threshold: the 12 records of a trace: the 10 moments over the cells with rho > threshold, record 10 the mass of
    every cell, record 11 the number of cells above the threshold (threshold = -inf takes every cell)."""
    rho = np.ascontiguousarray(rho_zyx, dtype=np.float64)
    assert rho.ndim == 3 and np.all(np.isfinite(rho))
    nz, ny, nx = rho.shape
    mant, expo = _mantissas(rho.ravel())
    idx = np.meshgrid(np.arange(nz, dtype=np.int64), np.arange(ny, dtype=np.int64), np.arange(nx, dtype=np.int64), indexing="ij")
    axes = [idx[2].ravel(), idx[1].ravel(), idx[0].ravel()]             # x, y, z
    scale = np.ones(rho.size, dtype=np.int64)
    denom = 1
    if weighted:                                                        # 8 * the trapezoid weight: an integer
        denom = 8
        for a, n in zip(axes, (nx, ny, nz)):
            scale *= np.where((a == 0) | (a == n - 1), 1, 2)
    keep = np.ones(rho.size, dtype=np.int64)
    if threshold is not None and threshold != -np.inf:
        keep = (rho.ravel() > threshold).astype(np.int64)
    weights = []
    for mono in MONOMIALS:
        w = scale * keep
        for a in mono:
            w = w * axes[a]
        weights.append(w)
    if threshold is not None:
        weights.append(np.ones(rho.size, dtype=np.int64))              # record 10: the mass of every cell
    sums, emin = _exact_dot(mant, expo, weights)
    abss = sums if mant.min() >= 0 else _exact_dot(np.abs(mant), expo, weights)[0]
    unit = Fraction(2) ** emin / denom
    moments, abs_sums = [s * unit for s in sums], [s * unit for s in abss]
    if threshold is not None:
        count = Fraction(int(keep.sum()))
        moments.append(count); abs_sums.append(count)
    return moments, abs_sums


def exact_com(moments, n):
    """The centre of mass analysis.com_from_moments forms, in exact arithmetic: (m_d / m_0 + 1/2) / n_d."""
    return [(moments[1 + d] / moments[0] + Fraction(1, 2)) / n[d] for d in range(3)]


def ratio_to_bound(got, exact, abs_sum, bound):
    """|got - exact| / (bound * sum |term|) in exact arithmetic, as a float: inside the bound where <= 1."""
    err = abs(Fraction(float(got)) - exact)
    lim = Fraction(bound) * abs_sum
    if lim == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / lim)


def _tree(a):
    """The shared-memory tree of block_reduce over the last axis (256 wide): a[t] += a[t + w], w = 128 .. 1."""
    a = a.copy()
    w = BLOCK // 2
    while w > 0:
        a[..., :w] += a[..., w:2 * w]
        w //= 2
    return a[..., 0]


def device_terms(rho_zyx, weighted=False, threshold=None):
    """terms[k][nz, ny, nx]: the rounded products the kernels add (k_moments; with a threshold trace_moments_body's 12)."""
    rho = np.asarray(rho_zyx, dtype=np.float64)
    nz, ny, nx = rho.shape
    z, y, x = [v.astype(np.float64) for v in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")]
    r = rho
    if weighted:
        r = rho.copy()
        for a, n in ((x, nx), (y, ny), (z, nz)):
            r = np.where((a == 0) | (a == n - 1), r * 0.5, r)
    mono = [np.ones_like(rho), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    if threshold is None:
        return [r * m for m in mono]
    keep = np.ones(rho.shape, dtype=bool) if threshold == -np.inf else rho > threshold
    return [np.where(keep, r * m, 0.0) for m in mono] + [rho, keep.astype(np.float64)]


def emulate_two_stage(terms_zyx, first_pass_only=False):
    """The sum of terms[nz, ny, nx] in the order of k_moments / trace_moments_body + k_plane_partials / k_trace_finish + the
    plane loop: rows at the padded pitch, blocks of 256 consecutive sites of the padded plane, the tree; every thread of
    stage 2 a 256-strided subsequence of the plane's block sums, the tree; the planes in sequence.
    first_pass_only: stage 2 cut to b < min(nbx, 256), the fault the wide-plane tests exist to catch."""
    t = np.asarray(terms_zyx, dtype=np.float64)
    nz, ny, nx = t.shape
    pitch = pitch_of(nx)
    nbx = blocks_per_plane(nx, ny)
    total = 0.0
    for z in range(nz):
        plane = np.zeros((ny, pitch))
        plane[:, :nx] = t[z]
        sites = np.zeros(nbx * BLOCK)
        sites[:pitch * ny] = plane.ravel()
        partial = _tree(sites.reshape(nbx, BLOCK))
        passes = 1 if first_pass_only else -(-nbx // BLOCK)
        strided = np.zeros(passes * BLOCK)
        m = min(nbx, passes * BLOCK)
        strided[:m] = partial[:m]
        v = np.zeros(BLOCK)
        for row in strided.reshape(passes, BLOCK):                      # b = thread, thread + 256, ...
            v = v + row
        total = total + _tree(v)
    return float(total)


def emulate_host_blocks(terms_zyx):
    """The sum of terms[nz, ny, nx] in the order of k_reduce + reduce5: the block sums added in sequence on the host."""
    t = np.asarray(terms_zyx, dtype=np.float64)
    nz, ny, nx = t.shape
    pitch = pitch_of(nx)
    nbx = blocks_per_plane(nx, ny)
    total = 0.0
    for z in range(nz):
        plane = np.zeros((ny, pitch))
        plane[:, :nx] = t[z]
        sites = np.zeros(nbx * BLOCK)
        sites[:pitch * ny] = plane.ravel()
        for p in _tree(sites.reshape(nbx, BLOCK)).tolist():
            total += p
    return total


# the shapes of tests/test_gpu_wide_planes.py, each the smallest of its kind: (shape, pitch, blocks per plane)
WIDE_SHAPES = [((512, 128, 3), 512, 256),      # the last width one pass of stage 2 serves (control)
               ((4112, 16, 3), 4112, 257),     # the first width with a second pass: thread 0 alone adds two blocks
               ((500, 135, 4), 512, 270),      # a second pass with 12 padded columns per row
               ((1000, 141, 2), 1008, 556)]    # three passes for threads 0-43, the last block ragged at 48 sites


def uniform_field(shape, seed):
    """[nz, ny, nx] i.i.d. uniform in [0.5, 1.5): every site and every block carries weight, no two sites are equal."""
    nx, ny, nz = shape
    return 0.5 + np.random.default_rng(seed).random((nz, ny, nx))
