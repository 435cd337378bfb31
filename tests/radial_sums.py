"""Radial traces: the order of the kernels' sums written out site by site, an exact reference and the error bound
(include/bflbm.h, "Radial traces": the definition and the order are stated there).  In the style of profile_sums.py.

    site_terms(x, d, r, pairs, radials)          the 1 + Q rounded terms of one site, Python floats
    emulate(fields, centre, delta, nbins, ...)   the record of k_radial_shells + k_radial_finish, bit for bit:
                                                 (counts[nbins], sums[Q, nbins])
    exact(fields, centre, delta, nbins, ...)     the sums of the rounded terms in fractions.Fraction, [1 + Q][nbins]
    abs_sums(...)                                sum |term| per entry, float [1 + Q, nbins]
    depth_bound(nx, ny, nz)                      d u / (1 - d u) against sum |term|
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                     # unit roundoff of a double
TILE = 256                         # sites of a tile
MAX_BINS = 128


def tiles_per_plane(nx, ny):
    return (nx * ny + TILE - 1) // TILE


def geometry(n, nq, nbins):
    """What bflbm_radial_geometry reports for the box n = (nx, ny, nz)."""
    return (nq, nbins, TILE, tiles_per_plane(n[0], n[1]))


def default_bins(n, delta):
    """The shells that cover half the box diagonal (the largest minimum-image distance), capped at 128."""
    return min(MAX_BINS, int(math.floor(0.5 * math.sqrt(n[0] ** 2 + n[1] ** 2 + n[2] ** 2) / delta)) + 1)


def depth_bound(nx, ny, nz):
    """d u / (1 - d u): the error of an entry against sum |rounded term| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2: a sum whose every term passes through at most d roundings, in any fixed order).  The
    additions a term passes through: at most 256 in its tile + the tiles of the plane + the nz planes.  The terms are
    taken as rounded (exact() adds the rounded products and projections), so the bound covers the additions only."""
    d = TILE + tiles_per_plane(nx, ny) + nz
    return d * U / (1.0 - d * U)


def _image(i, c, n):
    d = float(i) - c
    h = 0.5 * float(n)
    if d >= h:
        d = d - float(n)
    elif d < -h:
        d = d + float(n)
    return d


def _slots(pairs, radials):
    return [(int(a), int(b)) for a, b in pairs], [(-1 if w is None else int(w), tuple(int(c) for c in v)) for w, v in radials]


def site_terms(x, d, r, pairs, radials):
    """[1, x_0 .., x_a x_b .., radial terms ..] of a site with variables x, image vector d and distance r."""
    out = [1.0] + list(x) + [x[a] * x[b] for a, b in pairs]
    for w, (vx, vy, vz) in radials:
        p = 0.0 if r == 0.0 else ((x[vx] * d[0] + x[vy] * d[1]) + x[vz] * d[2]) / r
        out.append(p if w < 0 else x[w] * p)
    return out


def _walk(fields, centre, delta, nbins, pairs, radials):
    """Yields (z, tile, shell, terms) of every member site in the order z, s = y nx + x."""
    x = np.asarray(fields, dtype=np.float64)
    nv, nz, ny, nx = x.shape
    pairs, radials = _slots(pairs, radials)
    c = [float(v) for v in centre]
    delta = float(delta)
    flat = x.reshape(nv, nz, ny * nx)
    for z in range(nz):
        dz = _image(z, c[2], nz)
        cols = [flat[v, z].tolist() for v in range(nv)]
        for s in range(ny * nx):
            iy, ix = divmod(s, nx)
            d = (_image(ix, c[0], nx), _image(iy, c[1], ny), dz)
            rr = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if rr != rr:
                continue                                   # a NaN centre: no shell
            r = math.sqrt(rr)
            q = r / delta
            if not q < float(nbins):
                continue
            yield z, s // TILE, int(q), site_terms([col[s] for col in cols], d, r, pairs, radials)


def emulate(fields, centre, delta, nbins, pairs=(), radials=()):
    """(counts[nbins], sums[Q, nbins]) of fields[nvars, nz, ny, nx] in the kernels' order, in Python floats site by site:
    per (term, shell) the members of a tile added in ascending s from +0.0, the tiles of a plane in order, the planes
    in sequence."""
    x = np.asarray(fields, dtype=np.float64)
    nv, nz = x.shape[:2]
    nt = 1 + nv + len(pairs) + len(radials)
    total = [[0.0] * nbins for _ in range(nt)]
    plane = tile = None
    at = (-1, -1)

    def close_tile():
        for k in range(nt):
            for b in range(nbins):
                plane[k][b] = plane[k][b] + tile[k][b]

    def close_plane():
        for k in range(nt):
            for b in range(nbins):
                total[k][b] = total[k][b] + plane[k][b]

    for z, t, shell, terms in _walk(x, centre, delta, nbins, pairs, radials):
        if (z, t) != at:
            if tile is not None:
                close_tile()
            if z != at[0]:
                if plane is not None:
                    close_plane()
                plane = [[0.0] * nbins for _ in range(nt)]
            tile = [[0.0] * nbins for _ in range(nt)]
            at = (z, t)
        for k in range(nt):
            tile[k][shell] = tile[k][shell] + terms[k]
    if tile is not None:
        close_tile()
        close_plane()
    out = np.array(total, dtype=np.float64)
    return out[0], out[1:]


def exact(fields, centre, delta, nbins, pairs=(), radials=()):
    """[1 + Q][nbins] Fractions: the rounded terms of the member sites added exactly."""
    x = np.asarray(fields, dtype=np.float64)
    nt = 1 + x.shape[0] + len(pairs) + len(radials)
    out = [[Fraction(0)] * nbins for _ in range(nt)]
    for _, _, shell, terms in _walk(x, centre, delta, nbins, pairs, radials):
        for k in range(nt):
            out[k][shell] += Fraction(terms[k])
    return out


def abs_sums(fields, centre, delta, nbins, pairs=(), radials=()):
    x = np.asarray(fields, dtype=np.float64)
    nt = 1 + x.shape[0] + len(pairs) + len(radials)
    out = np.zeros((nt, nbins))
    for _, _, shell, terms in _walk(x, centre, delta, nbins, pairs, radials):
        for k in range(nt):
            out[k, shell] += abs(terms[k])
    return out


def ratio_to_bound(got, want, abs_sum, bound):
    """max over the entries of |got - want| / (bound * sum |term|) in exact arithmetic, as a float: inside the bound
    where <= 1.  got: float64 [1 + Q, nbins], want: Fractions [1 + Q][nbins]."""
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


def record(centre, counts, sums):
    """The sample of one replica as the device lays it out: [3 + (1 + Q) nbins]."""
    return np.concatenate([np.asarray(centre, dtype=np.float64), np.asarray(counts).ravel(), np.asarray(sums).ravel()])


# the boxes of the definition tests (nx, ny, nz) and what each exercises
BOXES = [(7, 9, 5),          # odd extents, a plane below one tile
         (32, 16, 3),        # two full tiles
         (33, 16, 3)]        # a short third tile


def centres(n):
    """{name: centre} of the definition tests for the box n.
    The ties d = +-n/2 of the minimum image need i - c = +-n/2 exactly: a half-integer centre meets them on the odd axes,
    an integer centre on the even ones, a low centre the tie +n/2 (which wraps to -n/2) and a high one the tie -n/2
    (which stays); "half" and "integer" hold one low and one high coordinate each."""
    return {"corner": (0.3, n[1] - 0.6, 0.45),             # all three axes wrap, with both signs
            "integer": (float(n[0] - 3), 3.0, 1.0),        # an r == 0 site: its radial term is +0.0
            "half": (0.5, n[1] - 1.5, 0.5),
            "nan": (float("nan"), 1.0, 1.0)}               # no site in any shell
