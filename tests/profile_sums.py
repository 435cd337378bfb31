"""Profile traces: the order of the kernels' sums written out site by site, an exact reference and the error bound
(include/bflbm.h, "Profile traces": the definition and the order are stated there).  In the style of mode_sums.py.

    terms(fields, pairs)             [Q, nz, ny, nx]: the variables, then the rounded products of the pairs
    emulate(fields, pairs, axis)     the record of k_profile_planes + k_profile_finish, bit for bit, [Q, n_a]
    exact(fields, pairs, axis)       the sums of the definition in fractions.Fraction, the products exact too
    abs_sums(fields, pairs, axis)    sum |term| per entry, float [Q, n_a]
    depth_bound(nx, ny, nz, axis)    d u / (1 - d u) against sum |term|
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                     # unit roundoff of a double
BLOCK = 256                        # threads of a workgroup
TILE = 2048                        # axis z: sites of a tile
LANES = 64                         # axis y: lanes that stride a row
CHUNK = 64                         # axis x: rows of a chunk
AXES = {"x": 0, "y": 1, "z": 2}


def tiles_per_plane(nx, ny):
    return (nx * ny + TILE - 1) // TILE


def geometry(n, nq, axis):
    """What bflbm_profile_geometry reports for the box n = (nx, ny, nz)."""
    axis = AXES.get(axis, axis)
    return (nq, n[axis], (CHUNK, LANES, TILE)[axis], tiles_per_plane(n[0], n[1]) if axis == 2 else n[axis])


def depth_bound(nx, ny, nz, axis):
    """d u / (1 - d u): the error of an entry against sum |term| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2: a sum whose every term passes through at most d roundings, in any fixed order).  d = 1 for
    the product of a pair + the additions a term passes through:
        axis z:  TILE / BLOCK = 8 of its thread + 8 levels of the tree + the tiles of the plane
        axis y:  ceil(nx / 64) turns of its lane + 6 levels of the tree + the nz planes
        axis x:  min(64, ny) rows of its chunk + ceil(ny / 64) chunks + the nz planes"""
    axis = AXES.get(axis, axis)
    if axis == 2:
        d = 1 + TILE // BLOCK + 8 + tiles_per_plane(nx, ny)
    elif axis == 1:
        d = 1 + (nx + LANES - 1) // LANES + 6 + nz
    else:
        d = 1 + min(CHUNK, ny) + (ny + CHUNK - 1) // CHUNK + nz
    return d * U / (1.0 - d * U)


def terms(fields, pairs):
    x = np.asarray(fields, dtype=np.float64)
    return np.concatenate([x] + [(x[a] * x[b])[None] for a, b in pairs], axis=0)


def _tree(v):
    """v[t] += v[t + w], w = len / 2 .. 1, on a list of floats; entry 0."""
    v = list(v)
    w = len(v) // 2
    while w:
        for t in range(w):
            v[t] = v[t] + v[t + w]
        w //= 2
    return v[0]


def _plane_z(p, nx, ny):
    """One partial per tile of the dense plane p[ny * nx]."""
    out = []
    for t0 in range(0, nx * ny, TILE):
        sums = [0.0] * BLOCK
        for t in range(BLOCK):
            for s in range(t0 + t, min(t0 + TILE, nx * ny), BLOCK):
                sums[t] = sums[t] + p[s]
        out.append(_tree(sums))
    return out


def _plane_y(p, nx, ny):
    """One partial per row."""
    out = []
    for y in range(ny):
        sums = [0.0] * LANES
        for lane in range(LANES):
            for x in range(lane, nx, LANES):
                sums[lane] = sums[lane] + p[y * nx + x]
        out.append(_tree(sums))
    return out


def _plane_x(p, nx, ny):
    """One partial per column."""
    out = []
    for x in range(nx):
        total = 0.0
        for c0 in range(0, ny, CHUNK):
            chunk = 0.0
            for y in range(c0, min(c0 + CHUNK, ny)):
                chunk = chunk + p[y * nx + x]
            total = total + chunk
        out.append(total)
    return out


def emulate(fields, pairs, axis):
    """float64 [Q, n_a]: the record of fields[nvars, nz, ny, nx] in the kernels' order, in Python floats site by site."""
    axis = AXES.get(axis, axis)
    t = terms(fields, pairs)
    nq, nz, ny, nx = t.shape
    out = np.zeros((nq, (nx, ny, nz)[axis]))
    for q in range(nq):
        planes = [t[q, z].reshape(-1).tolist() for z in range(nz)]
        if axis == 2:
            for z in range(nz):
                s = 0.0
                for part in _plane_z(planes[z], nx, ny):
                    s = s + part
                out[q, z] = s
        else:
            parts = [(_plane_y if axis == 1 else _plane_x)(planes[z], nx, ny) for z in range(nz)]
            for i in range(out.shape[1]):
                s = 0.0
                for z in range(nz):
                    s = s + parts[z][i]
                out[q, i] = s
    return out


def exact(fields, pairs, axis):
    """[Q][n_a] Fractions: the sums of the definition over the doubles of the fields, products and sums exact."""
    axis = AXES.get(axis, axis)
    x = np.asarray(fields, dtype=np.float64)
    nv, nz, ny, nx = x.shape
    F = [[Fraction(v) for v in x[k].reshape(-1).tolist()] for k in range(nv)]
    vols = F + [[a * b for a, b in zip(F[pa], F[pb])] for pa, pb in pairs]
    shape = (nz, ny, nx)
    keep = 2 - axis                                        # the array axis of the lattice axis
    out = []
    for vol in vols:
        sums = [Fraction(0)] * shape[keep]
        for s, v in enumerate(vol):
            idx = (s // (ny * nx), (s // nx) % ny, s % nx)[keep]
            sums[idx] += v
        out.append(sums)
    return out


def abs_sums(fields, pairs, axis):
    axis = AXES.get(axis, axis)
    x = np.abs(np.asarray(fields, dtype=np.float64))
    t = np.concatenate([x] + [(x[a] * x[b])[None] for a, b in pairs], axis=0)
    return t.sum(axis=tuple(k for k in (1, 2, 3) if k != 3 - axis))


def ratio_to_bound(got, want, abs_sum, bound):
    """max over the entries of |got - want| / (bound * sum |term|) in exact arithmetic, as a float: inside the bound
    where <= 1.  got: float64 [Q, n_a], want: Fractions [Q][n_a]."""
    worst = 0.0
    for q in range(len(want)):
        for i in range(len(want[q])):
            err = abs(Fraction(float(got[q, i])) - want[q][i])
            lim = Fraction(bound) * Fraction(float(abs_sum[q, i]))
            if lim == 0:
                worst = max(worst, 0.0 if err == 0 else float("inf"))
            else:
                worst = max(worst, float(err / lim))
    return worst


# the boxes of the definition tests (nx, ny, nz) and what each exercises
BOXES = [(7, 9, 5),          # odd site counts, a plane below 256 sites
         (64, 32, 3),        # one full tile of 2048 sites
         (66, 32, 3),        # a second, short tile
         (65, 3, 2), (130, 3, 2),      # second and third lane turns of a row
         (3, 65, 2), (3, 130, 2)]      # second and third row chunks
