"""Mode traces: the order of the kernels' sums in numpy, an exact reference and the error bound (include/bflbm.h, "Mode
traces": the definition and the order are stated there).  In the style of exact_sums.py.

    phase_table(lib, n)            T_n of bflbm_modes_phases: the library's own table, float64 [n, 2]
    emulate(field, modes, tables)  the record of k_modes_project + k_modes_finish, bit for bit
    exact(field, modes, tables)    the same sums over the same tables in fractions.Fraction: no rounding at all
    longdouble_projection(...)     the same in longdouble, for larger fields
    depth_bound(nx, ny, nz)        d u / (1 - d u) against sum |a|
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                     # unit roundoff of a double
BLOCK = 256                        # threads of a workgroup
TILE = 2048                        # sites of a tile (bflbm_modes_geometry reports it)
PER_THREAD = TILE // BLOCK


def tiles_per_plane(nx, ny):
    return (nx * ny + TILE - 1) // TILE


def depth_bound(nx, ny, nz):
    """d u / (1 - d u): the error of a record's component against sum |a| (Higham, Accuracy and Stability of Numerical
    Algorithms, section 4.2: a sum whose every term passes through at most d roundings, in any fixed order).
    d = 8 + the additions a term passes through inside its plane + nz.  The 8: 3 roundings forming the term (two for a
    component of T_nx T_ny, one for a times it), 2 for the z phase applied to the plane's sum, and 3 of slack for
    |T_nx T_ny T_nz| differing from 1 (three table entries, each within 2^-52 of the unit circle).  Inside its plane a
    term passes through the thread's PER_THREAD additions, the 8 levels of the tree and the plane's tile additions."""
    d = 8 + PER_THREAD + 8 + tiles_per_plane(nx, ny) + nz
    return d * U / (1.0 - d * U)


def phase_table(lib, n):
    t = np.empty((n, 2))
    assert lib.bflbm_modes_phases(n, t.ctypes.data) == 0
    return t


def tables_of(lib, n):
    """(T_nx, T_ny, T_nz) of the box n = (nx, ny, nz)."""
    return tuple(phase_table(lib, m) for m in n)


def _indices(m, n):
    """j[i] = ((m mod n) i) mod n."""
    return ((m % n) * np.arange(n)) % n


def _tree(v):
    """The tree of block_reduce over the last axis (256 wide): v[t] += v[t + w], w = 128 .. 1."""
    v = v.copy()
    w = BLOCK // 2
    while w:
        v[..., :w] = v[..., :w] + v[..., w:2 * w]
        w //= 2
    return v[..., 0]


def emulate(field_zyx, modes, tables):
    """complex128 [nmodes]: the record of field_zyx[nz, ny, nx] in the kernels' order.  Per plane and tile the thread t
    adds a * (T_nx[jx] T_ny[jy]) of the sites t, t + 256, ... starting from 0, the tree adds the 256 sums, the tiles are
    added in order, the plane's sum is multiplied by T_nz[jz], the planes are added in sequence."""
    a = np.asarray(field_zyx, dtype=np.float64)
    nz, ny, nx = a.shape
    tx, ty, tz = tables
    tiles = tiles_per_plane(nx, ny)
    padded = np.zeros((nz, tiles * TILE))
    padded[:, :nx * ny] = a.reshape(nz, nx * ny)
    out = np.empty(len(modes), dtype=np.complex128)
    for i, (mx, my, mz) in enumerate(np.asarray(modes).tolist()):
        px, py = tx[_indices(mx, nx)], ty[_indices(my, ny)]
        pr = px[None, :, 0] * py[:, None, 0] - px[None, :, 1] * py[:, None, 1]                           # [ny, nx]: px * py
        pi = px[None, :, 0] * py[:, None, 1] + px[None, :, 1] * py[:, None, 0]
        comp = []
        for p in (pr, pi):
            ph = np.zeros(tiles * TILE)
            ph[:nx * ny] = p.reshape(-1)
            term = (padded * ph[None, :]).reshape(nz, tiles, PER_THREAD, BLOCK)
            acc = np.zeros((nz, tiles, BLOCK))
            for k in range(PER_THREAD):
                acc = acc + term[:, :, k, :]
            blocks = _tree(acc)                            # [nz, tiles]
            plane = np.zeros(nz)
            for t in range(tiles):
                plane = plane + blocks[:, t]
            comp.append(plane)
        sr, si = comp
        bz = tz[_indices(mz, nz)]
        zr = sr * bz[:, 0] - si * bz[:, 1]
        zi = sr * bz[:, 1] + si * bz[:, 0]
        re = im = 0.0
        for z in range(nz):
            re = re + zr[z]
            im = im + zi[z]
        out[i] = complex(re, im)
    return out


def exact(field_zyx, modes, tables):
    """[(re, im)] per mode as Fractions: sum of a (T_nx[jx] T_ny[jy] T_nz[jz]) over the doubles of the field and of the
    library's tables, in exact arithmetic.  For the small boxes of the tests."""
    a = np.asarray(field_zyx, dtype=np.float64)
    nz, ny, nx = a.shape
    F = [[[Fraction(float(v)) for v in row] for row in plane] for plane in a]
    T = [[(Fraction(float(c)), Fraction(float(s))) for c, s in t] for t in tables]
    out = []
    for mx, my, mz in np.asarray(modes).tolist():
        jx, jy, jz = _indices(mx, nx), _indices(my, ny), _indices(mz, nz)
        re = im = Fraction(0)
        for z in range(nz):
            zr, zi = T[2][jz[z]]
            pr = pi = Fraction(0)
            for y in range(ny):
                yr, yi = T[1][jy[y]]
                rr = ri = Fraction(0)
                for x in range(nx):
                    xr, xi = T[0][jx[x]]
                    v = F[z][y][x]
                    rr += v * xr
                    ri += v * xi
                pr += rr * yr - ri * yi
                pi += rr * yi + ri * yr
            re += pr * zr - pi * zi
            im += pr * zi + pi * zr
        out.append((re, im))
    return out


def longdouble_projection(field_zyx, modes, tables):
    """[(re, im)] per mode in longdouble: the sums of exact() with 64-bit mantissas, whose own error (some 1e-19 of
    sum |a|) is three orders below the bound; for the fields that are too many for Fractions."""
    a = np.asarray(field_zyx, dtype=np.longdouble)
    nz, ny, nx = a.shape
    T = [t.astype(np.longdouble) for t in tables]
    out = []
    for mx, my, mz in np.asarray(modes).tolist():
        px, py, pz = T[0][_indices(mx, nx)], T[1][_indices(my, ny)], T[2][_indices(mz, nz)]
        rr, ri = (a * px[:, 0]).sum(axis=2), (a * px[:, 1]).sum(axis=2)                   # [nz, ny]
        pr, pi = (rr * py[:, 0] - ri * py[:, 1]).sum(axis=1), (rr * py[:, 1] + ri * py[:, 0]).sum(axis=1)
        out.append(((pr * pz[:, 0] - pi * pz[:, 1]).sum(), (pr * pz[:, 1] + pi * pz[:, 0]).sum()))
    return out


def ratio_to_bound(got, want, abs_sum, bound):
    """max over the two components of |got - want| / (bound * sum |a|) in exact arithmetic, as a float: inside the bound
    where <= 1.  got: a complex double, want: (re, im) Fractions."""
    lim = Fraction(bound) * Fraction(float(abs_sum))
    want = [w if isinstance(w, Fraction) else Fraction(*[int(v) for v in np.longdouble(w).as_integer_ratio()]) for w in want]
    err = max(abs(Fraction(float(got.real)) - want[0]), abs(Fraction(float(got.imag)) - want[1]))
    if lim == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / lim)


def issue_modes(n):
    """The wavevectors of the definition tests."""
    nx, ny, nz = n
    return np.array([(1, 0, 0), (-3, 2, 1), (nx // 2, ny // 2, nz // 2), (0, 0, 0), (5, -4, -2)], dtype=np.int64)
