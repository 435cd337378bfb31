"""Droplet observables of the validation notebooks, as host-side post-processing of a density field.

The reference analyses its plotfiles in Droplet_Fluctuation.ipynb / Surface_Tension.ipynb (cell 3 there
defines the quantities; its C++ twin is LBM_hydrovs.H:117-335, off by default, main_run_job.cpp:111).
These are the same definitions re-stated on numpy arrays so that the numbers the notebooks record can
be checked directly (tests/test_gpu_fullsize.py).  The *_from_moments functions evaluate the same
quantities from the 20 raw moments the device reduces (BinaryLBM.droplet_moments, csrc/bflbm_droplet.h),
so that no field has to leave the GPU; BinaryLBM.fit_droplet is the device version of fit_droplet.

Conventions of the notebooks: coordinates are cell centres (i + 1/2)/n of a unit box; fields are
indexed [x, y, z] there -- pass `rho_xyz = rho.transpose(2, 1, 0)` for an array in (z, y, x) order.
"""
import functools
import math

import numpy as np


def _centres(shape):
    return [(np.arange(n) + 0.5) / n for n in shape]


def centre_of_mass(rho_xyz):
    """sum(r rho)/sum(rho) with cell-centred coordinates."""
    x, y, z = _centres(rho_xyz.shape)
    m = rho_xyz.sum()
    return np.array([(rho_xyz * x[:, None, None]).sum(), (rho_xyz * y[None, :, None]).sum(),
                     (rho_xyz * z[None, None, :]).sum()]) / m


def radial_profile(rho_xyz, r0=None):
    """Flattened densities and their distance from r0 (default: the centre of mass)."""
    r0 = centre_of_mass(rho_xyz) if r0 is None else np.asarray(r0)
    x, y, z = _centres(rho_xyz.shape)
    r = np.sqrt((x[:, None, None] - r0[0]) ** 2 + (y[None, :, None] - r0[1]) ** 2 + (z[None, None, :] - r0[2]) ** 2)
    return rho_xyz.ravel(), r.ravel()


def fit_droplet(rho_xyz, r0=None):
    """Least-squares fit of rho(r) = hi - (hi - lo)/2 (1 + tanh((r - R)/W)); returns (hi, lo, R, W).
    Start values as in the notebook: (max rho, min rho, 0.5, 0.5)."""
    from scipy.optimize import curve_fit

    def profile(r, hi, lo, radius, width):
        return hi - (hi - lo) / 2 * (1 + np.tanh((r - radius) / width))

    rho, r = radial_profile(rho_xyz, r0)
    popt, _ = curve_fit(profile, r, rho, p0=[rho.max(), rho.min(), 0.5, 0.5])
    return tuple(popt)


def mass_covariance(rho_xyz):
    """Second central moments of the mass distribution, trapezoid-weighted like the notebook
    (end planes count half), about the (unweighted) centre of mass."""
    x, y, z = _centres(rho_xyz.shape)
    wt = np.ones(rho_xyz.shape)
    for ax in range(3):
        sl = [slice(None)] * 3
        for end in (0, -1):
            sl[ax] = end
            wt[tuple(sl)] *= 0.5
    r0 = centre_of_mass(rho_xyz)
    w = rho_xyz * wt
    m = w.sum()
    d = [x[:, None, None] - r0[0], y[None, :, None] - r0[1], z[None, None, :] - r0[2]]
    c = np.empty((3, 3))
    for a in range(3):
        for b in range(a, 3):
            c[a, b] = c[b, a] = (d[a] * d[b] * w).sum() / m
    return c


def principal_axes(rho_xyz, radius):
    """Eigen-decomposition of the mass covariance and the semi-axes of the equal-volume ellipsoid."""
    ev, vec = np.linalg.eig(mass_covariance(rho_xyz))
    axes = np.array([ev[k] ** (1. / 3.) * radius / (ev[(k + 1) % 3] * ev[(k + 2) % 3]) ** (1. / 6.) for k in range(3)])
    return axes, ev, vec


def msd(r, max_lag):
    """Mean squared displacement of trajectories r[..., T, 3] (e.g. Trace.com() with the time axis moved next to last):
    msd[..., k] = mean over t of |r[t + k] - r[t]|^2 over all frame pairs of lag k = 0 ... max_lag (msd[..., 0] = 0)."""
    r = np.asarray(r, dtype=np.float64)
    nt = r.shape[-2]
    if not 0 <= max_lag < nt:
        raise ValueError(f"msd: max_lag {max_lag} needs more than {nt} frames")
    out = np.zeros(r.shape[:-2] + (max_lag + 1,))
    for k in range(1, max_lag + 1):
        d = r[..., k:, :] - r[..., :nt - k, :]
        out[..., k] = (d * d).sum(axis=-1).mean(axis=-1)
    return out


def interface_heights(field_zyx, level, window=None):
    """The numpy restatement of the interface trace (include/bflbm.h, "Interface traces", is the definition): for every
    column of field_zyx[nz, ny, nx] the height of the first rising (d(z-1) < level <= d(z)) and of the first falling
    (d(z-1) >= level > d(z)) pair of the window [z_lo, z_hi) (default: all planes), scanned upward without a wrap,
    h = (z-1) + (level - d(z-1)) / (d(z) - d(z-1)).  Returns [2, ny, nx] (0 rising, 1 falling), NaN without a crossing."""
    d = np.asarray(field_zyx, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"interface_heights: a field [nz, ny, nx], got shape {d.shape}")
    z_lo, z_hi = (0, d.shape[0]) if window is None else (int(window[0]), int(window[1]))
    if not (0 <= z_lo and z_hi <= d.shape[0] and z_hi - z_lo >= 2):
        raise ValueError(f"interface_heights: window [{z_lo}, {z_hi}) of {d.shape[0]} planes")
    level = np.float64(level)
    a, b = d[z_lo:z_hi - 1], d[z_lo + 1:z_hi]                # d(z-1), d(z) of the pairs z = z_lo+1 ... z_hi-1
    out = np.full((2,) + d.shape[1:], np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, hit in enumerate(((a < level) & (level <= b), (a >= level) & (level > b))):   # a NaN compares false
            first = np.argmax(hit, axis=0)[None]             # the first pair that crosses (0 where none does)
            lo, hi = np.take_along_axis(a, first, axis=0)[0], np.take_along_axis(b, first, axis=0)[0]
            h = (z_lo + first[0]).astype(np.float64) + (level - lo) / (hi - lo)
            out[k] = np.where(hit.any(axis=0), h, np.nan)
    return out


def capillary_spectrum(h, axes=(-1,)):
    """<|h_q|^2> of a height series h[T, ...] (Flat_Interface.ipynb cell 9, for one or both in-plane axes): the time mean
    of every column is removed, numpy's unnormalised DFT is taken over `axes`, and |h_q|^2 is averaged over T.
    Returns (spectrum of shape h.shape[1:], tuple of the wave numbers q = 2 pi fftfreq(n) of every axis in `axes`)."""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim < 2:
        raise ValueError("capillary_spectrum: h[T, ...] with at least one in-plane axis")
    axes = tuple(a if a >= 0 else h.ndim + a for a in axes)
    if any(not 1 <= a < h.ndim for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"capillary_spectrum: axes {axes} of an array with {h.ndim} dimensions (axis 0 is time)")
    hq = np.fft.fftn(h - h.mean(axis=0), axes=axes)
    return (np.abs(hq) ** 2).mean(axis=0), tuple(2 * np.pi * np.fft.fftfreq(h.shape[a]) for a in axes)


# ---- droplet shape modes: the numpy restatement of the shape trace (include/bflbm.h, "Shape traces") and its projection ----
SHAPE_DIRECTIONS = {"falling": 0, "rising": 1}


def ray_nodes(ntheta, nphi):
    """Directions and weights of a product quadrature on the sphere: ntheta Gauss-Legendre nodes in cos(theta) times nphi
    equally spaced phi = 2 pi (k + 1/2) / nphi.  Returns (dirs[ntheta * nphi, 3], weights[ntheta * nphi]), theta-major; the
    weights sum to 4 pi, and products of spherical harmonics of total degree < min(2 ntheta, nphi) integrate exactly.
    These are the rays of a ShapeTrace (the r(theta, phi) grid of Droplet_Fluctuation.ipynb cell 32)."""
    ntheta, nphi = int(ntheta), int(nphi)
    if ntheta < 1 or nphi < 1:
        raise ValueError(f"ray_nodes: ntheta {ntheta} and nphi {nphi} must be >= 1")
    ct, wt = np.polynomial.legendre.leggauss(ntheta)
    st = np.sqrt(1.0 - ct * ct)
    phi = 2.0 * np.pi * (np.arange(nphi) + 0.5) / nphi
    dirs = np.empty((ntheta, nphi, 3))
    dirs[..., 0] = st[:, None] * np.cos(phi)[None, :]
    dirs[..., 1] = st[:, None] * np.sin(phi)[None, :]
    dirs[..., 2] = ct[:, None]
    weights = np.repeat(wt * (2.0 * np.pi / nphi), nphi)
    return dirs.reshape(-1, 3), weights


def _density_at(d, px, py, pz):
    """The trilinear density of the definition at the points (px, py, pz) of a field d[nz, ny, nx]."""
    nz, ny, nx = d.shape
    with np.errstate(invalid="ignore"):
        ok = (np.abs(px) < 2.0 ** 30) & (np.abs(py) < 2.0 ** 30) & (np.abs(pz) < 2.0 ** 30)     # false for a NaN
    qx, qy, qz = np.where(ok, px, 0.0), np.where(ok, py, 0.0), np.where(ok, pz, 0.0)
    flx, fly, flz = np.floor(qx), np.floor(qy), np.floor(qz)
    fx, fy, fz = qx - flx, qy - fly, qz - flz
    x0, y0, z0 = flx.astype(np.int64) % nx, fly.astype(np.int64) % ny, flz.astype(np.int64) % nz   # numpy's % wraps negatives up
    x1, y1, z1 = (x0 + 1) % nx, (y0 + 1) % ny, (z0 + 1) % nz
    c00 = d[z0, y0, x0] + fx * (d[z0, y0, x1] - d[z0, y0, x0])
    c10 = d[z0, y1, x0] + fx * (d[z0, y1, x1] - d[z0, y1, x0])
    c01 = d[z1, y0, x0] + fx * (d[z1, y0, x1] - d[z1, y0, x0])
    c11 = d[z1, y1, x0] + fx * (d[z1, y1, x1] - d[z1, y1, x0])
    c0 = c00 + fy * (c10 - c00)
    c1 = c01 + fy * (c11 - c01)
    return np.where(ok, c0 + fz * (c1 - c0), np.nan)


def droplet_radii(field_zyx, centre, dirs, level, step, nsteps, direction="falling"):
    """The numpy restatement of the shape trace (include/bflbm.h, "Shape traces", is the definition), operation for
    operation: along every unit vector dirs[j] from `centre` (cell indices x, y, z) the trilinearly interpolated, periodic
    field_zyx[nz, ny, nx] is sampled at t_k = k step, k = 0 ... nsteps, and the first pair that falls (d_{k-1} >= level >
    d_k) or rises (d_{k-1} < level <= d_k) through the level gives r = step ((k-1) + linear interpolation).  Returns
    r[ndir], NaN where a ray has no such pair or the centre is not finite.  It stands for the marching-cubes surface of
    Droplet_Fluctuation.ipynb cell 32, seen from the centre of mass."""
    d = np.asarray(field_zyx, dtype=np.float64)
    if d.ndim != 3:
        raise ValueError(f"droplet_radii: a field [nz, ny, nx], got shape {d.shape}")
    u = np.asarray(dirs, dtype=np.float64)
    if u.ndim != 2 or u.shape[1] != 3:
        raise ValueError(f"droplet_radii: dirs [ndir, 3], got shape {u.shape}")
    rising = SHAPE_DIRECTIONS.get(direction, direction)
    if rising not in (0, 1):
        raise ValueError(f"droplet_radii: direction {direction!r}, expected 'falling' (0) or 'rising' (1)")
    nsteps = int(nsteps)
    if not (nsteps >= 1 and np.isfinite(step) and step > 0):
        raise ValueError(f"droplet_radii: step {step} must be finite and > 0, nsteps {nsteps} >= 1")
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    level, step = np.float64(level), np.float64(step)
    r = np.full(len(u), np.nan)
    found = np.zeros(len(u), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        prev = _density_at(d, c[0] + np.float64(0.0) * u[:, 0], c[1] + np.float64(0.0) * u[:, 1], c[2] + np.float64(0.0) * u[:, 2])
        for k in range(1, nsteps + 1):
            t = np.float64(k) * step
            cur = _density_at(d, c[0] + t * u[:, 0], c[1] + t * u[:, 1], c[2] + t * u[:, 2])
            if rising:
                hit, num, den = (prev < level) & (level <= cur), level - prev, cur - prev
            else:
                hit, num, den = (prev >= level) & (level > cur), prev - level, prev - cur
            new = hit & ~found                                   # a NaN density compares false
            r[new] = (step * (np.float64(k - 1) + num / den))[new]
            found |= new
            prev = cur
    return r


def real_harmonics(dirs, lmax):
    """Orthonormal real spherical harmonics Y[ndir, (lmax + 1)^2] at the unit vectors dirs[ndir, 3], in the order l = 0 ...
    lmax, m = -l ... l (m < 0: the sin(|m| phi) partner, m > 0: cos(m phi)), without the Condon-Shortley phase.  Built by
    Cartesian recurrences, no angles: c_m + i s_m = (ux + i uy)^m; Q_m^m = (2m-1)!!, Q_{m+1}^m = (2m+1) uz Q_m^m,
    Q_l^m = ((2l-1) uz Q_{l-1}^m - (l+m-1) Q_{l-2}^m) / (l-m); Y_lm = N_lm Q_l^|m| {sqrt(2) s_|m|, 1, sqrt(2) c_m} with
    N_lm^2 = (2l+1) (l-|m|)! / (4 pi (l+|m|)!).  The basis of the zeta_lm of Droplet_Fluctuation.ipynb cells 38 and 41."""
    u = np.asarray(dirs, dtype=np.float64)
    lmax = int(lmax)
    if u.ndim != 2 or u.shape[1] != 3 or lmax < 0:
        raise ValueError(f"real_harmonics: dirs [ndir, 3] and lmax >= 0, got shape {u.shape} and lmax {lmax}")
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    Y = np.empty((len(u), (lmax + 1) ** 2))
    cm, sm = np.ones(len(u)), np.zeros(len(u))
    qmm = 1.0
    for m in range(lmax + 1):
        if m > 0:
            cm, sm = cm * ux - sm * uy, cm * uy + sm * ux
            qmm *= 2 * m - 1
        q2, q1 = None, np.full(len(u), qmm)                      # Q_{l-2}^m, Q_{l-1}^m
        for l in range(m, lmax + 1):
            if l == m:
                q = q1
            elif l == m + 1:
                q = (2 * m + 1) * uz * q1
            else:
                q = ((2 * l - 1) * uz * q1 - (l + m - 1) * q2) / (l - m)
            if l > m:
                q2, q1 = q1, q
            norm = math.sqrt((2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                Y[:, l * l + l] = norm * q
            else:
                Y[:, l * l + l + m] = math.sqrt(2.0) * norm * q * cm
                Y[:, l * l + l - m] = math.sqrt(2.0) * norm * q * sm
    return Y


def shape_modes(r, dirs, weights, lmax):
    """a_lm = sum_j w_j r_j Y_lm(u_j) of radii r[..., ndir] on the rays dirs with quadrature weights (ray_nodes): the
    shape coefficients a[..., (lmax + 1)^2] in the order of real_harmonics, a_00 = sqrt(4 pi) times the mean radius.  A
    frame with a NaN radius gives NaN modes.  These are the zeta_lm(t) of Droplet_Fluctuation.ipynb cells 38 and 41, whose
    variance the theory gives as kBT / (gamma (l-1)(l+2))."""
    r = np.asarray(r, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    Y = real_harmonics(dirs, lmax)
    if r.shape[-1:] != w.shape or w.shape != (Y.shape[0],):
        raise ValueError(f"shape_modes: r[..., ndir], dirs[ndir, 3] and weights[ndir] disagree: {r.shape}, {Y.shape[0]}, {w.shape}")
    a = (r.reshape(-1, 1, len(w)) * w) @ Y                       # one product per frame: a NaN stays in its own frame
    return a.reshape(r.shape[:-1] + (Y.shape[1],))


# ---- binned structure factors: the numpy restatement of the spectrum trace (include/bflbm.h, "Spectrum traces") ----------
SPECTRUM_KINDS = {"shell": 0, "x": 1, "y": 2, "z": 3}


def _shell_of(k2, w):
    """The integer s >= 0 with (2s-1)^2 w^2 <= 4 k2 < (2s+1)^2 w^2, in Python integers."""
    s = (math.isqrt(4 * k2) // w + 1) // 2
    while s > 0 and (2 * s - 1) ** 2 * w * w > 4 * k2:
        s -= 1
    while (2 * s + 1) ** 2 * w * w <= 4 * k2:
        s += 1
    return s


@functools.lru_cache(maxsize=8)
def _spectrum_bins(n, kind, zero_avg):
    nx, ny, nz = n
    kx, ky, kz = [np.minimum(np.arange(m), m - np.arange(m)).astype(np.int64) for m in (nx, ny, nz)]   # |k| in fftn's order
    if kind == 0:
        L = math.lcm(nx, ny, nz)
        if 12 * (L // 2) ** 2 >= 2 ** 63:
            raise ValueError(f"spectrum_bins: lcm{n} = {L} is too large for shells: 12 (L/2)^2 must fit in 63 bits")
        w = L // max(n)
        k2 = ((kz * (L // nz)) ** 2)[:, None, None] + ((ky * (L // ny)) ** 2)[None, :, None] + ((kx * (L // nx)) ** 2)[None, None, :]
        values, inverse = np.unique(k2, return_inverse=True)
        bins = np.array([_shell_of(int(v), w) for v in values], dtype=np.int64)[inverse].reshape(k2.shape)
    else:
        bins = np.broadcast_to([kx[None, None, :], ky[None, :, None], kz[:, None, None]][kind - 1], (nz, ny, nx)).copy()
    nbins = int(bins.max()) + 1
    if zero_avg:
        bins[0, 0, 0] = -1
    keep = bins.ravel() >= 0
    count = np.bincount(bins.ravel()[keep], minlength=nbins).astype(np.int64)
    if kind == 0:
        fx, fy, fz = kx / nx, ky / ny, kz / nz
        q_mode = 2.0 * np.pi * np.sqrt((fx * fx)[None, None, :] + (fy * fy)[None, :, None] + (fz * fz)[:, None, None])
        order = np.argsort(bins.ravel()[keep], kind="stable")
        sorted_q = q_mode.ravel()[keep][order].astype(np.longdouble)
        q = np.full(nbins, np.nan)
        filled = np.flatnonzero(count)
        starts = (np.cumsum(count) - count)[filled]
        q[filled] = (np.add.reduceat(sorted_q, starts) / count[filled].astype(np.longdouble)).astype(np.float64)
    else:
        q = 2.0 * np.pi * np.arange(nbins) / float(n[kind - 1])
    for a in (bins, count, q):
        a.setflags(write=False)
    return bins, count, q


def spectrum_bins(n, kind, zero_avg=True):
    """The bins of a spectrum trace on an n = (nx, ny, nz) lattice; kind "shell" (0), "x" (1), "y" (2) or "z" (3).
    Returns (bin[nz, ny, nx] of every full-spectrum mode in numpy's fftn layout, -1 for the k = 0 mode that zero_avg
    leaves out; count[nbins] int64; q[nbins]).  The shell of a mode is decided in Python integers (math.isqrt)."""
    n = (n, n, n) if np.isscalar(n) else tuple(int(v) for v in n)
    kind = SPECTRUM_KINDS.get(kind, kind)
    if kind not in (0, 1, 2, 3):
        raise ValueError(f"spectrum_bins: kind {kind!r}, expected one of {sorted(SPECTRUM_KINDS)} or 0..3")
    return _spectrum_bins(n, int(kind), bool(zero_avg))


def binned_spectrum(a_zyx, b_zyx, kind, zero_avg=True, scale=1.0):
    """sum[bin] of S_ab(k) = scale Re(a^(k) conj(b^(k))) / N over the full spectrum (numpy fftn) of two fields [nz, ny, nx]."""
    a, b = np.asarray(a_zyx, dtype=np.float64), np.asarray(b_zyx, dtype=np.float64)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError(f"binned_spectrum: two fields [nz, ny, nx] of one shape, got {a.shape} and {b.shape}")
    bins, count, _ = spectrum_bins(a.shape[::-1], kind, zero_avg)
    s = (scale * np.fft.fftn(a) * np.conj(np.fft.fftn(b))).real / a.size
    keep = bins.ravel() >= 0
    return np.bincount(bins.ravel()[keep], weights=s.ravel()[keep], minlength=len(count))


def domain_length(q, s_mean):
    """L = 2 pi sum_{bin >= 1} S / sum_{bin >= 1} q S, the inverse first moment of a binned spectrum s_mean[..., nbins]
    (sums / count); bins without modes (NaN) do not enter."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s_mean, dtype=np.float64)
    ok = np.isfinite(q[1:]) & np.isfinite(s[..., 1:])
    top = np.where(ok, s[..., 1:], 0.0).sum(axis=-1)
    return 2.0 * np.pi * top / np.where(ok, q[1:] * s[..., 1:], 0.0).sum(axis=-1)


# ---- the same observables from the device-reduced raw moments (BinaryLBM.droplet_moments) ----------------
# m[0:10] = sum rho {1, x, y, z, xx, xy, xz, yy, yz, zz} in cell indices, m[10:20] trapezoid-weighted.

def fourier_modes(field_zyx, modes):
    """a^(m) of include/bflbm.h, "Mode traces", in numpy: field_zyx[..., nz, ny, nx] real, modes[nmodes, 3] integer
    (mx, my, mz), any integers; returns complex128 [..., nmodes] = fftn(field)[mz % nz, my % ny, mx % nx].  np.exp
    phases and numpy's summation order: equal to the library's records up to rounding, not bit for bit."""
    a = np.asarray(field_zyx, dtype=np.float64)
    m = np.asarray(modes)
    if a.ndim < 3 or m.ndim != 2 or m.shape[1] != 3 or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"fourier_modes: field[..., nz, ny, nx] and integer modes[nmodes, 3], got {a.shape} and {m.shape} of {m.dtype}")
    nz, ny, nx = a.shape[-3:]
    if len(m) == 0:
        return np.empty(a.shape[:-3] + (0,), dtype=np.complex128)
    ex, ey, ez = [np.exp(-2j * np.pi * (((m[:, d] % n)[None, :] * np.arange(n)[:, None]) % n) / n)     # [n, nmodes]
                  for d, n in enumerate((nx, ny, nz))]
    rows = np.ascontiguousarray(a).reshape(-1, nx)
    t = (rows @ ex.real + 1j * (rows @ ex.imag)).reshape(a.shape[:-1] + (len(m),))      # x summed: [..., nz, ny, nmodes]
    t = (t * ey).sum(axis=-2)                              # y summed: [..., nz, nmodes]
    return (t * ez).sum(axis=-2)


def time_correlation(a, b=None, max_lag=None):
    """C[lag] = mean over t of a[t + lag] conj(b[t]), lag = 0 .. max_lag, along the leading axis (b None: a itself; max_lag
    None: len(a) - 1); the other axes pass through.  Every lag averages over the len(a) - lag pairs it has."""
    a = np.asarray(a)
    b = a if b is None else np.asarray(b)
    if a.shape != b.shape or a.ndim < 1 or len(a) < 1:
        raise ValueError(f"time_correlation: two series of one shape with a leading time axis, got {a.shape} and {b.shape}")
    nt = len(a)
    max_lag = nt - 1 if max_lag is None else int(max_lag)
    if not 0 <= max_lag < nt:
        raise ValueError(f"time_correlation: max_lag {max_lag} outside 0 .. {nt - 1}")
    return np.stack([(a[lag:] * np.conj(b[:nt - lag])).mean(axis=0) for lag in range(max_lag + 1)])


def field_statistics(frames, pairs=()):
    """Field statistics of include/bflbm.h in numpy, operation for operation: frames[N][nvars][nz][ny][nx] in recording
    order (one replica), pairs of variable slots (a, b).  Returns a dict of `first`[nvars, ...], `sum`[nvars, ...] (the
    sequential sum), `prod`[npairs, ...] (sum over the frames, from +0.0, of the product of the deviations from the first
    frame), `mean` = sum * (1.0 / N) and `cov` = prod * (1.0 / N) - (mean[a] - first[a]) * (mean[b] - first[b]), and `N`."""
    x = np.asarray(frames, dtype=np.float64)
    if x.ndim < 2 or len(x) < 1:
        raise ValueError(f"field_statistics: frames[N >= 1][nvars][...], got shape {x.shape}")
    pairs = [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if not (0 <= a < x.shape[1] and 0 <= b < x.shape[1]):
            raise ValueError(f"field_statistics: pair ({a}, {b}) outside the {x.shape[1]} variables")
    n = len(x)
    first = x[0].copy()
    total = x[0].copy()
    prod = np.zeros((len(pairs),) + x.shape[2:])
    for t in range(1, n):
        total = total + x[t]
        dev = x[t] - first
        for p, (a, b) in enumerate(pairs):
            prod[p] = prod[p] + dev[a] * dev[b]
    inv = 1.0 / float(n)
    mean = total * inv
    cov = np.empty_like(prod)
    for p, (a, b) in enumerate(pairs):
        cov[p] = prod[p] * inv - (mean[a] - first[a]) * (mean[b] - first[b])
    return dict(first=first, sum=total, prod=prod, mean=mean, cov=cov, N=n)


def field_statistics_ensemble(replicas):
    """The ensemble values of include/bflbm.h, "Field statistics", from the field_statistics of the replicas 0 ... B-1
    (all of N frames): `mean` = the replicas' sum added in that order from 0, times 1.0 / (B N); `cov` = the replicas' cov
    added in that order from 0, times 1.0 / B (the mean within-replica covariance)."""
    reps = list(replicas)
    if not reps or any(r["N"] != reps[0]["N"] for r in reps):
        raise ValueError("field_statistics_ensemble: the statistics of B >= 1 replicas over the same number of frames")
    total = np.zeros_like(reps[0]["sum"])
    cov = np.zeros_like(reps[0]["cov"])
    for r in reps:
        total = total + r["sum"]
        cov = cov + r["cov"]
    b = float(len(reps))
    return dict(mean=total * (1.0 / (b * float(reps[0]["N"]))), cov=cov * (1.0 / b))


# ---- plane profiles: the numpy restatement of the profile trace (include/bflbm.h, "Profile traces") and the pressure profile ----
PROFILE_TILE, PROFILE_LANES, PROFILE_CHUNK = 2048, 64, 64      # what bflbm_profile_geometry reports per axis z, y, x


def _tree(v):
    """v[..., t] += v[..., t + w], w = n/2 ... 1, over the last axis (a power of two wide); the entry 0."""
    v = v.copy()
    w = v.shape[-1] // 2
    while w:
        v[..., :w] = v[..., :w] + v[..., w:2 * w]
        w //= 2
    return v[..., 0]


def plane_profiles(fields, pairs=(), axis=2):
    """sums[Q, n_a] of include/bflbm.h, "Profile traces", in numpy, operation for operation and in the header's order:
    fields[nvars, nz, ny, nx], pairs a list of (a, b) variable slots, axis 0 (x), 1 (y), 2 (z) or "x", "y", "z".  Entry
    (q, i): the sum over the lattice plane i normal to the axis of variable q, or of the product of the pair q - nvars."""
    x = np.asarray(fields, dtype=np.float64)
    axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
    if x.ndim != 4 or axis not in (0, 1, 2):
        raise ValueError(f"plane_profiles: fields[nvars, nz, ny, nx] and an axis in 0..2, got {x.shape} and {axis!r}")
    nv, nz, ny, nx = x.shape
    pairs = [(int(a), int(b)) for a, b in pairs]
    if any(not (0 <= a < nv and 0 <= b < nv) for a, b in pairs):
        raise ValueError(f"plane_profiles: a pair slot outside the {nv} variables: {pairs}")
    terms = np.concatenate([x] + [(x[a] * x[b])[None] for a, b in pairs], axis=0)        # [Q, nz, ny, nx]
    nq = len(terms)
    if axis == 2:
        tiles = (nx * ny + PROFILE_TILE - 1) // PROFILE_TILE
        padded = np.zeros((nq, nz, tiles * PROFILE_TILE))
        padded[..., :nx * ny] = terms.reshape(nq, nz, nx * ny)
        padded = padded.reshape(nq, nz, tiles, PROFILE_TILE // 256, 256)
        acc = np.zeros((nq, nz, tiles, 256))
        for k in range(PROFILE_TILE // 256):               # thread t: the sites t, t + 256, ...
            acc = acc + padded[..., k, :]
        part = _tree(acc)                                  # [Q, nz, tiles]
        out = np.zeros((nq, nz))
        for t in range(tiles):
            out = out + part[..., t]
        return out
    if axis == 1:
        turns = (nx + PROFILE_LANES - 1) // PROFILE_LANES
        padded = np.zeros((nq, nz, ny, turns * PROFILE_LANES))
        padded[..., :nx] = terms
        padded = padded.reshape(nq, nz, ny, turns, PROFILE_LANES)
        acc = np.zeros((nq, nz, ny, PROFILE_LANES))
        for k in range(turns):                             # lane l: x = l, l + 64, ...
            acc = acc + padded[..., k, :]
        part = _tree(acc)                                  # [Q, nz, ny]
    else:
        part = np.zeros((nq, nz, nx))
        for c0 in range(0, ny, PROFILE_CHUNK):
            chunk = np.zeros((nq, nz, nx))
            for y in range(c0, min(c0 + PROFILE_CHUNK, ny)):
                chunk = chunk + terms[:, :, y, :]
            part = part + chunk                            # the chunks in order
    out = np.zeros((nq, part.shape[-1]))
    for z in range(nz):                                    # the planes in sequence, as the last step
        out = out + part[:, z]
    return out


# ---- histograms: the numpy restatement of the histogram trace (include/bflbm.h, "Histogram traces") ----
HIST_MAX_BINS, HIST_MAX_PAIRS, HIST_MAX_COUNTERS = 4096, 4, 16384


def histogram_blocks(nbins, pairs=()):
    """(C, [(offset, length)]) of a sample of include/bflbm.h, "Histogram traces": per variable nbins_v bins + below,
    above, nan; then per pair (a, b) of slots nbins_a x nbins_b cells + outside."""
    nbins = [int(n) for n in nbins]
    lengths = [n + 3 for n in nbins] + [nbins[int(a)] * nbins[int(b)] + 1 for a, b in pairs]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(int).tolist()
    return offsets[-1], list(zip(offsets[:-1], lengths))


def _bin_indices(x, lo, hi, nbins):
    """The counter of every value within its variable's block: 0 .. nbins-1 a bin, nbins below, nbins + 1 above,
    nbins + 2 nan."""
    scale = np.float64(nbins) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - np.float64(lo)                             # the subtraction first ...
        t = d * scale                                      # ... the multiplication second
        nan, below, above = np.isnan(t), t < 0.0, t >= np.float64(nbins)
    inside = ~(nan | below | above)
    idx = np.where(inside, t, 0.0).astype(np.int64)        # truncation
    idx[above] = nbins + 1
    idx[below] = nbins
    idx[nan] = nbins + 2
    return idx


def field_histograms(fields, lo, hi, nbins, pairs=()):
    """counts[C] int64 of include/bflbm.h, "Histogram traces", in numpy, operation for operation (float64 subtract,
    multiply, compare, truncate): fields[nvars, ...] of one replica, lo[nvars], hi[nvars], nbins[nvars], pairs a list of
    (a, b) of variable slots, a != b.  The layout is histogram_blocks(nbins, pairs)."""
    x = np.asarray(fields, dtype=np.float64)
    nv = len(x)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    nbins = [int(n) for n in np.asarray(nbins).reshape(-1)]
    pairs = [(int(a), int(b)) for a, b in pairs]
    if x.ndim < 2 or not (1 <= nv <= 8) or not (len(lo) == len(hi) == len(nbins) == nv):
        raise ValueError(f"field_histograms: fields[1..8 variables, ...] with lo, hi, nbins per variable, got {x.shape}, {len(lo)}, {len(hi)}, {len(nbins)}")
    for v in range(nv):
        if not (np.isfinite(lo[v]) and np.isfinite(hi[v]) and hi[v] > lo[v]):
            raise ValueError(f"field_histograms: variable slot {v}: the range needs finite lo < hi (got {lo[v]}, {hi[v]})")
        if not (1 <= nbins[v] <= HIST_MAX_BINS):
            raise ValueError(f"field_histograms: variable slot {v}: 1..{HIST_MAX_BINS} bins (got {nbins[v]})")
        with np.errstate(over="ignore", divide="ignore"):
            scale = np.float64(nbins[v]) / (hi[v] - lo[v])
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError(f"field_histograms: variable slot {v}: the scale nbins / (hi - lo) = {scale} is not finite and positive")
    if len(pairs) > HIST_MAX_PAIRS or any(not (0 <= a < nv and 0 <= b < nv) or a == b for a, b in pairs):
        raise ValueError(f"field_histograms: 0..{HIST_MAX_PAIRS} pairs of two different slots of the {nv} variables: {pairs}")
    total, blocks = histogram_blocks(nbins, pairs)
    if total > HIST_MAX_COUNTERS:
        raise ValueError(f"field_histograms: {total} counters exceed {HIST_MAX_COUNTERS}")
    idx = [_bin_indices(x[v].reshape(-1), lo[v], hi[v], nbins[v]) for v in range(nv)]
    out = np.zeros(total, dtype=np.int64)
    for v in range(nv):
        off, n = blocks[v]
        out[off:off + n] = np.bincount(idx[v], minlength=n)
    for p, (a, b) in enumerate(pairs):
        off, n = blocks[nv + p]
        both = (idx[a] < nbins[a]) & (idx[b] < nbins[b])
        cell = np.where(both, idx[a] * nbins[b] + idx[b], n - 1)
        out[off:off + n] = np.bincount(cell, minlength=n)
    return out


def histogram_moments(counts, lo, hi):
    """(mean, variance) of the in-range counts[..., nbins] from the bin centres lo + (k + 1/2) (hi - lo) / nbins; NaN
    where no site is in range.  Every value lies within half a bin width of its centre, so the mean is within half a
    bin width of the mean of the in-range values."""
    c = np.asarray(counts, dtype=np.float64)
    n = c.shape[-1]
    centres = float(lo) + (np.arange(n) + 0.5) * ((float(hi) - float(lo)) / n)
    with np.errstate(invalid="ignore", divide="ignore"):
        total = c.sum(axis=-1)
        mean = (c * centres).sum(axis=-1) / total
        var = (c * (centres - mean[..., None]) ** 2).sum(axis=-1) / total
    return mean, var


# ---- morphology: the numpy restatement of the morphology trace (include/bflbm.h, "Morphology traces") ----
MORPH_MAX_LEVELS = 8
MORPH_SIDES = {"above": 0, "below": 1}


def minkowski_counts(field_zyx, levels, side="above"):
    """counts[nlevels, 4] int64 of include/bflbm.h, "Morphology traces", in numpy: N3, N2, N1, N0, the cubes, faces,
    edges and vertices of the union of the closed voxels of the sites with field >= level (side "above" or 0) or
    field < level (side "below" or 1) on the periodic box field_zyx[nz, ny, nx], for 1..8 finite levels.  A NaN occupies
    nothing on either side."""
    v = np.asarray(field_zyx, dtype=np.float64)
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if v.ndim != 3 or v.size == 0:
        raise ValueError(f"minkowski_counts: a field [nz, ny, nx], got shape {v.shape}")
    if lv.ndim != 1 or not (1 <= len(lv) <= MORPH_MAX_LEVELS):
        raise ValueError(f"minkowski_counts: 1..{MORPH_MAX_LEVELS} levels (got shape {lv.shape})")
    if not np.isfinite(lv).all():
        raise ValueError(f"minkowski_counts: the levels must be finite (got {lv.tolist()})")
    if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
        raise ValueError(f"minkowski_counts: side {side!r}, expected 'above' (0) or 'below' (1)")
    below = bool(MORPH_SIDES.get(side, side))
    out = np.empty((len(lv), 4), dtype=np.int64)

    def nxt(a, axis):                                      # the periodic successor along an axis: 0 z, 1 y, 2 x
        return np.roll(a, -1, axis=axis)

    for l, t in enumerate(lv):
        with np.errstate(invalid="ignore"):
            o = (v < t) if below else (v >= t)
        ox, oy, oz = o | nxt(o, 2), o | nxt(o, 1), o | nxt(o, 0)
        oyz, oxz, oxy = oy | nxt(oy, 0), ox | nxt(ox, 0), ox | nxt(ox, 1)
        oxyz = oxy | nxt(oxy, 0)
        out[l] = (o.sum(), ox.sum() + oy.sum() + oz.sum(), oyz.sum() + oxz.sum() + oxy.sum(), oxyz.sum())
    return out


def minkowski_functionals(counts):
    """[..., 4] int64: V = N3, S = -6 N3 + 2 N2, 2B = 3 N3 - 2 N2 + N1, chi = -N3 + N2 - N1 + N0 of counts[..., 4]
    (N3, N2, N1, N0): the volume in cells, the area in cell faces, twice the mean breadth in cell edges and the Euler
    characteristic."""
    c = np.asarray(counts)
    if c.ndim < 1 or c.shape[-1] != 4 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"minkowski_functionals: integer counts [..., 4], got shape {c.shape} of {c.dtype}")
    c = c.astype(np.int64)
    n3, n2, n1, n0 = (c[..., k] for k in range(4))
    return np.stack([n3, -6 * n3 + 2 * n2, 3 * n3 - 2 * n2 + n1, -n3 + n2 - n1 + n0], axis=-1)


def morphology_length(counts, nsites):
    """[...]: nsites / S of counts[..., 4], the real-space domain size L = V_box / S; NaN where S = 0."""
    s = minkowski_functionals(counts)[..., 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s != 0, float(nsites) / s, np.nan)


# ---- chords: the numpy restatement of the chord trace (include/bflbm.h, "Chord traces") ----
CHORD_MAX_LENGTH = 4096


def chord_blocks(max_length=64):
    """The layout of a level's W = 1 + 3 (3 + M) words: {"W": W, "occupied": 0, "x" | "y" | "z": {"chords": i,
    "spanning": i, "long_sites": i, "hist": slice of h[1..M]}}."""
    m = int(max_length)
    if not 1 <= m <= CHORD_MAX_LENGTH:
        raise ValueError(f"chord_blocks: max_length in 1..{CHORD_MAX_LENGTH} (got {max_length})")
    out = {"W": 1 + 3 * (3 + m), "occupied": 0}
    for a, name in enumerate("xyz"):
        at = 1 + a * (3 + m)
        out[name] = {"chords": at, "spanning": at + 1, "long_sites": at + 2, "hist": slice(at + 3, at + 3 + m)}
    return out


def _chord_axis(axis):
    if axis in ("x", "y", "z"):
        return axis
    if axis in (0, 1, 2):
        return "xyz"[axis]
    raise ValueError(f"chord axis {axis!r}, expected 'x', 'y', 'z' or 0..2")


def chord_counts(field_zyx, levels, side="above", max_length=64):
    """counts[nlevels, W] int64 of include/bflbm.h, "Chord traces", in numpy: per level the occupied sites, then per axis
    x, y, z the chords, the spanning lines, long_sites and the bins h[1..M] of the maximal runs of sites with
    field >= level (side "above" or 0) or field < level (side "below" or 1) along the periodic lines of
    field_zyx[nz, ny, nx], for 1..8 finite levels.  A NaN occupies nothing on either side.  Per line the runs' first and
    last sites are found by differences with the rolled line; the k-th first site pairs with the k-th last site, after
    the last site of a run through the seam has been moved past the line's end."""
    v = np.asarray(field_zyx, dtype=np.float64)
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if v.ndim != 3 or v.size == 0:
        raise ValueError(f"chord_counts: a field [nz, ny, nx], got shape {v.shape}")
    if lv.ndim != 1 or not (1 <= len(lv) <= MORPH_MAX_LEVELS):
        raise ValueError(f"chord_counts: 1..{MORPH_MAX_LEVELS} levels (got shape {lv.shape})")
    if not np.isfinite(lv).all():
        raise ValueError(f"chord_counts: the levels must be finite (got {lv.tolist()})")
    if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
        raise ValueError(f"chord_counts: side {side!r}, expected 'above' (0) or 'below' (1)")
    below = bool(MORPH_SIDES.get(side, side))
    m = int(max_length)
    layout = chord_blocks(m)
    out = np.zeros((len(lv), layout["W"]), dtype=np.int64)
    for l, t in enumerate(lv):
        with np.errstate(invalid="ignore"):
            o = (v < t) if below else (v >= t)
        out[l, 0] = o.sum()
        for name, ax in (("x", 2), ("y", 1), ("z", 0)):
            blk = layout[name]
            lines = np.moveaxis(o, ax, -1).reshape(-1, o.shape[ax])
            n = lines.shape[1]
            full = lines.all(axis=1)
            out[l, blk["spanning"]] = full.sum()
            lines = lines[~full]
            first = lines & ~np.roll(lines, 1, axis=1)              # a run's first site: its predecessor is unoccupied
            last = lines & ~np.roll(lines, -1, axis=1)              # a run's last site: its successor is unoccupied
            fl, fp = np.nonzero(first)                                # in line order, then position order
            ll, lp = np.nonzero(last)
            opens = np.flatnonzero(np.r_[True, ll[1:] != ll[:-1]]) if len(ll) else ll      # a line's least last site
            seam = opens[lines[ll[opens], 0] & lines[ll[opens], -1]]  # ... belongs to the run through the seam where both ends are occupied
            lp[seam] += n
            key = ll * (2 * n) + lp
            key.sort()
            length = key - (fl * (2 * n) + fp) + 1
            out[l, blk["chords"]] = len(length)
            out[l, blk["long_sites"]] = length[length >= m].sum()
            out[l, blk["hist"]] = np.bincount(np.minimum(length, m), minlength=m + 1)[1:]
    return out


def chord_mean_length(counts, n):
    """[..., 3]: the mean chord (V - n_a spanning) / chords along x, y, z of counts[..., W] for the box n = (nx, ny, nz);
    NaN where an axis has no chord."""
    c = np.asarray(counts)
    if c.ndim < 1 or (c.shape[-1] - 1) % 3 or c.shape[-1] < 13 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"chord_mean_length: integer counts [..., 1 + 3 (3 + M)], got shape {c.shape} of {c.dtype}")
    if len(n) != 3:
        raise ValueError(f"chord_mean_length: n = (nx, ny, nz), got {n!r}")
    layout = chord_blocks((c.shape[-1] - 1) // 3 - 3)
    v = c[..., 0].astype(np.float64)
    out = []
    for name, na in zip("xyz", n):
        chords = c[..., layout[name]["chords"]].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(chords > 0, (v - float(na) * c[..., layout[name]["spanning"]]) / chords, np.nan))
    return np.stack(out, axis=-1)


# ---- coarse fields: the numpy restatement of the coarse trace (include/bflbm.h, "Coarse traces") ----
COARSE_MAX_VARS, COARSE_MAX_PAIRS, COARSE_MAX_BLOCK_X = 8, 16, 256


def _coarse_triple(what, v):
    try:
        t = tuple(int(x) for x in v)
    except TypeError:
        t = ()
    if len(t) != 3:
        raise ValueError(f"coarse_fields: {what} is three integers (x, y, z), got {v!r}")
    return t


def coarse_fields(fields, pairs=(), origin=(0, 0, 0), extent=None, block=(1, 1, 1)):
    """sums[Q, c_z, c_y, c_x] of include/bflbm.h, "Coarse traces", in numpy, operation for operation and in the header's
    order: fields[nvars, nz, ny, nx], pairs a list of (a, b) variable slots, origin, extent and block as (x, y, z)
    (extent None: from the origin to the end of the box).  Entry (q, Z, Y, X): the sum over the block of variable q, or of
    the product of the pair q - nvars; the window is periodic."""
    x = np.asarray(fields, dtype=np.float64)
    if x.ndim != 4 or not 1 <= x.shape[0] <= COARSE_MAX_VARS or min(x.shape) < 1:
        raise ValueError(f"coarse_fields: fields[nvars, nz, ny, nx] with 1..{COARSE_MAX_VARS} variables, got {x.shape}")
    nv, nz, ny, nx = x.shape
    n = (nx, ny, nz)
    pairs = [(int(a), int(b)) for a, b in pairs]
    if len(pairs) > COARSE_MAX_PAIRS:
        raise ValueError(f"coarse_fields: 0..{COARSE_MAX_PAIRS} pairs, got {len(pairs)}")
    if any(not (0 <= a < nv and 0 <= b < nv) for a, b in pairs):
        raise ValueError(f"coarse_fields: a pair slot outside the {nv} variables: {pairs}")
    o = _coarse_triple("origin", origin)
    w = tuple(na - oa for na, oa in zip(n, o)) if extent is None else _coarse_triple("extent", extent)
    b = _coarse_triple("block", block)
    for a in range(3):
        if not 0 <= o[a] < n[a]:
            raise ValueError(f"coarse_fields: origin[{'xyz'[a]}] = {o[a]} outside 0..{n[a] - 1}")
    for a in range(3):
        if not 1 <= w[a] <= n[a]:
            raise ValueError(f"coarse_fields: extent[{'xyz'[a]}] = {w[a]} outside 1..{n[a]}")
    for a in range(3):
        if b[a] < 1 or w[a] % b[a]:
            raise ValueError(f"coarse_fields: block[{'xyz'[a]}] = {b[a]} must be >= 1 and divide the extent {w[a]}")
    if b[0] > COARSE_MAX_BLOCK_X:
        raise ValueError(f"coarse_fields: block[x] = {b[0]} exceeds {COARSE_MAX_BLOCK_X}")
    ix, iy, iz = [(o[a] + np.arange(w[a])) % n[a] for a in range(3)]                     # the periodic window
    win = x[:, iz][:, :, iy][:, :, :, ix]                                               # [nvars, w_z, w_y, w_x]
    terms = np.concatenate([win] + [(win[p] * win[q])[None] for p, q in pairs], axis=0)
    cx, cy, cz = [w[a] // b[a] for a in range(3)]
    terms = terms.reshape(len(terms), cz, b[2], cy, b[1], cx, b[0])
    col = np.zeros((len(terms), cz, cy, cx, b[0]))
    for dz in range(b[2]):                                 # per fine column: dz, then dy
        for dy in range(b[1]):
            col = col + terms[:, :, dz, :, dy, :, :]
    out = np.zeros((len(terms), cz, cy, cx))
    for dx in range(b[0]):                                 # then the columns of a block, left to right
        out = out + col[..., dx]
    return out


def coarse_block_variance(sum_a, sum_b, sum_ab, block_sites):
    """The covariance of a and b within every block from the block sums of a, b and a * b over block_sites = b_x b_y b_z
    sites each: the mean of the product minus the product of the means (a is b: the block variance).  Arrays of one
    shape."""
    sa, sb, sab = (np.asarray(v, dtype=np.float64) for v in (sum_a, sum_b, sum_ab))
    if not (sa.shape == sb.shape == sab.shape) or int(block_sites) < 1:
        raise ValueError(f"coarse_block_variance: three arrays of one shape and block_sites >= 1, got {sa.shape}, {sb.shape}, {sab.shape}, {block_sites!r}")
    m = float(int(block_sites))
    return sab / m - (sa / m) * (sb / m)


# ---- lag records: the numpy restatement of the lag trace (include/bflbm.h, "Lag traces") ----
LAG_MAX_VARS, LAG_MAX_PAIRS, LAG_MAX_ORIGINS = 8, 8, 16


def lag_slots(nsamples, norigins, origin_stride):
    """held[nsamples, R] int64: the sample whose origin slot r holds at sample n, after sample n has taken its own (-1: the
    slot is empty).  Sample n with n % E == 0 takes an origin into slot (n / E) % R."""
    ns, r, e = int(nsamples), int(norigins), int(origin_stride)
    if ns < 0 or not 1 <= r <= LAG_MAX_ORIGINS or e < 1:
        raise ValueError(f"lag_slots: nsamples >= 0, 1..{LAG_MAX_ORIGINS} origins and a stride >= 1, got {nsamples!r}, {norigins!r}, {origin_stride!r}")
    held = np.full((ns, r), -1, dtype=np.int64)
    for n in range(ns):
        if n > 0:
            held[n] = held[n - 1]
        if n % e == 0:
            held[n, (n // e) % r] = n
    return held


def _z_sum(profile):
    """The planes z = 0 .. nz-1 of sums[Q, nz] in sequence, from +0.0."""
    out = np.zeros(profile.shape[0])
    for z in range(profile.shape[1]):
        out = out + profile[:, z]
    return out


def lag_record(frames, steps, pairs, norigins, origin_stride=1, persist_slot=-1, persist_level=0.0):
    """(now[n, nvars], origin_steps[n, R] int64, alive[n, R] int64, corr[n, R, npairs]) of include/bflbm.h, "Lag traces",
    in numpy, operation for operation and in the header's order: frames[n, nvars, nz, ny, nx] the observed variables at
    the samples of one replica, steps[n] its step counter at each, pairs a list of (a, b) variable slots.  Every double
    sum is plane_profiles(..., axis=2) summed over z in sequence."""
    x = np.asarray(frames, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.int64)
    if x.ndim != 5 or not 1 <= x.shape[1] <= LAG_MAX_VARS or steps.shape != x.shape[:1]:
        raise ValueError(f"lag_record: frames[n, nvars, nz, ny, nx] with 1..{LAG_MAX_VARS} variables and steps[n], got {x.shape} and {steps.shape}")
    ns, nv = x.shape[:2]
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not 1 <= len(pairs) <= LAG_MAX_PAIRS or any(not (0 <= a < nv and 0 <= b < nv) for a, b in pairs):
        raise ValueError(f"lag_record: 1..{LAG_MAX_PAIRS} pairs of slots within the {nv} variables, got {pairs}")
    ps = int(persist_slot)
    if not -1 <= ps < nv or (ps >= 0 and not np.isfinite(persist_level)):
        raise ValueError(f"lag_record: persist_slot in -1..{nv - 1} and a finite level, got {persist_slot!r}, {persist_level!r}")
    held = lag_slots(ns, norigins, origin_stride)
    r = held.shape[1]
    now = np.zeros((ns, nv))
    origin_steps = np.full((ns, r), -1, dtype=np.int64)
    alive = np.full((ns, r), -1, dtype=np.int64)
    corr = np.full((ns, r, len(pairs)), np.nan)
    bits = np.zeros((r,) + x.shape[2:], dtype=bool)        # a site's bit per slot
    lagged = [(a, nv + b) for a, b in pairs]               # the current variables, then the origin's
    level = np.float64(persist_level)
    for n in range(ns):
        now[n] = _z_sum(plane_profiles(x[n], (), axis=2))
        with np.errstate(invalid="ignore"):
            side = x[n, ps] >= level if ps >= 0 else None  # a NaN: false
        for k in range(r):
            o = held[n, k]
            if o < 0:
                continue
            origin_steps[n, k] = steps[o]
            corr[n, k] = _z_sum(plane_profiles(np.concatenate([x[n], x[o]]), lagged, axis=2))[2 * nv:]
            if ps >= 0:
                if o == n:
                    bits[k] = True                         # the origin is taken: every site's bit is set
                with np.errstate(invalid="ignore"):
                    bits[k] &= side == (x[o, ps] >= level)
                alive[n, k] = np.count_nonzero(bits[k])
    return now, origin_steps, alive, corr


def lag_average(steps, origin_steps, values):
    """(lags, mean[nlags], origins[nlags] int64): values[n, R] of a lag record averaged over the origins by
    lag = steps[n] - origin_steps[n, r], in steps; empty slots (origin_step < 0) and NaN values are left out."""
    steps = np.asarray(steps, dtype=np.int64)
    osteps = np.asarray(origin_steps, dtype=np.int64)
    v = np.asarray(values, dtype=np.float64)
    if osteps.ndim != 2 or steps.shape != osteps.shape[:1] or v.shape != osteps.shape:
        raise ValueError(f"lag_average: steps[n], origin_steps[n, R] and values[n, R], got {steps.shape}, {osteps.shape}, {v.shape}")
    lag = steps[:, None] - osteps
    use = (osteps >= 0) & ~np.isnan(v)
    lags = np.unique(lag[use])
    mean = np.array([v[use & (lag == d)].mean() for d in lags], dtype=np.float64)
    count = np.array([np.count_nonzero(use & (lag == d)) for d in lags], dtype=np.int64)
    return lags, mean, count


def lag_connected(steps, origin_steps, corr, now_a, now_b, nsites):
    """corr[n, R] of the pair (a, b) minus now_a[n] * now_b[the origin's own sample] / nsites: the connected part.  NaN
    where the origin's own sample is not in the record (an empty slot, or a window read without it)."""
    steps = np.asarray(steps, dtype=np.int64)
    osteps = np.asarray(origin_steps, dtype=np.int64)
    c, na, nb = (np.asarray(v, dtype=np.float64) for v in (corr, now_a, now_b))
    if osteps.ndim != 2 or c.shape != osteps.shape or not (steps.shape == na.shape == nb.shape == osteps.shape[:1]) or int(nsites) < 1:
        raise ValueError(f"lag_connected: steps[n], origin_steps[n, R], corr[n, R], now_a[n], now_b[n], got {steps.shape}, {osteps.shape}, {c.shape}, {na.shape}, {nb.shape}")
    out = np.full(c.shape, np.nan)
    where = {int(s): n for n, s in reversed(list(enumerate(steps)))}   # the first sample of a step
    for n in range(osteps.shape[0]):
        for k in range(osteps.shape[1]):
            o = where.get(int(osteps[n, k])) if osteps[n, k] >= 0 else None
            if o is not None and o <= n:
                out[n, k] = c[n, k] - na[n] * nb[o] / float(int(nsites))
    return out


# ---- moment records: the numpy restatement of the moment trace (include/bflbm.h, "Moment traces") ----
MOMENT_MODES, MOMENT_WORDS = 19, 95
# b[a]: the norms of the basis vectors of the moment transform (LBM_d3q19.H:56-76), the weight of mode a in equipartition
MOMENT_NORMS = (1.0, 1. / 3., 1. / 3., 1. / 3., 2. / 3., 4. / 3., 4. / 9., 1. / 9., 1. / 9., 1. / 9.,
                2. / 3., 2. / 3., 2. / 3., 2. / 9., 2. / 9., 2. / 9., 2.0, 4. / 3., 4. / 9.)
_MOMENT_NAMES = ("rho", "jx", "jy", "jz",                               # density and momentum
                 "s_tr", "s_xx", "s_ww", "s_xy", "s_yz", "s_xz",        # stress: trace, 3 xx - cc, yy - zz, the three shears
                 "g_jx", "g_jy", "g_jz", "g_hx", "g_hy", "g_hz",        # ghost vectors: (3 cc - 5) c, and the plane differences
                 "g_tr", "g_xx", "g_ww")                                # ghost scalars: the fourth-order partners of s_tr, s_xx, s_ww


def moment_names():
    """The 19 modes of one fluid in the order of the transform (LBM_d3q19.H:100-156): rho, jx, jy, jz; the six stress
    moments s_tr (c.c - 1 summed: the bulk mode), s_xx (3 cx^2 - c.c), s_ww (cy^2 - cz^2), s_xy, s_yz, s_xz; the ghost
    moments g_jx..g_jz ((3 c.c - 5) c), g_hx..g_hz (the differences between the planes' momenta) and g_tr, g_xx, g_ww."""
    return list(_MOMENT_NAMES)


def _quad(q0, q1, q2, q3):
    """The four signed sums of a coordinate plane's diagonal populations, accumulated left to right (csrc/bflbm_site.h, d_quad)."""
    u = q0 - q1 + q2 - q3
    v = q0 - q1 - q2 + q3
    w = q0 + q1 - q2 - q3
    t = q0 + q1 + q2 + q3
    return u, v, w, t


def moments_of(f):
    """m[19, ...] = moments(f[19, ...]) with the association of csrc/bflbm_site.h's d_moments, which is the reference's
    (LBM_d3q19.H:100-156): the doubles equal the oracle's orc_moments."""
    f = np.asarray(f, dtype=np.float64)
    if f.ndim < 1 or f.shape[0] != MOMENT_MODES:
        raise ValueError(f"moments_of: populations[19, ...], got shape {f.shape}")
    dif = [f[1 + 2 * a] - f[2 + 2 * a] for a in range(3)]
    tot = [f[1 + 2 * a] + f[2 + 2 * a] for a in range(3)]
    xy_u, xy_v, xy_w, xy_t = _quad(f[7], f[8], f[9], f[10])             # u: x-momentum, v: y-momentum
    yz_u, yz_v, yz_w, yz_t = _quad(f[11], f[12], f[13], f[14])          # u: y-momentum, v: z-momentum
    xz_u, xz_v, xz_w, xz_t = _quad(f[15], f[16], f[17], f[18])          # u: x-momentum, v: z-momentum
    rest = f[0]
    shell1 = tot[0] + tot[1] + tot[2]
    shell2 = xy_t + yz_t + xz_t
    m = np.empty_like(f)
    m[0] = rest + shell1 + shell2
    m[1] = dif[0] + xy_u + xz_u
    m[2] = dif[1] + yz_u + xy_v
    m[3] = dif[2] + xz_v + yz_v
    m[4] = shell2 - rest
    m[5] = 3. * tot[0] - shell1 + shell2 - 3. * yz_t
    m[6] = tot[1] - tot[2] + xy_t - xz_t
    m[7] = xy_w
    m[8] = yz_w
    m[9] = xz_w
    m[10] = m[1] - 3. * dif[0]
    m[11] = m[2] - 3. * dif[1]
    m[12] = m[3] - 3. * dif[2]
    m[13] = xy_u - xz_u
    m[14] = yz_u - xy_v
    m[15] = xz_v - yz_v
    m[16] = m[0] - 3. * shell1
    m[17] = shell1 - 3. * tot[0] + shell2 - 3. * yz_t
    m[18] = tot[2] - tot[1] + xy_t - xz_t
    return m


def moment_terms(f, g):
    """terms[95, nz, ny, nx]: what every site adds to the 95 words of a sample: the 38 moments (19 fluid + a), their
    squares and the 19 products mf_a mg_a, each product rounded once."""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if f.ndim != 4 or f.shape[0] != MOMENT_MODES or g.shape != f.shape:
        raise ValueError(f"moment_record: f[19, nz, ny, nx] and g of the same shape, got {f.shape} and {g.shape}")
    mf, mg = moments_of(f), moments_of(g)
    return np.concatenate([mf, mg, mf * mf, mg * mg, mf * mg], axis=0)


def moment_record(f, g):
    """sums[95] of include/bflbm.h, "Moment traces", in numpy, operation for operation and in the header's order: f, g the
    populations [19, nz, ny, nx] that populations() returns.  Every sum is plane_profiles(..., axis=2) of its term summed
    over z in sequence: the lag trace's order for `now`.  Taken plane by plane, so a large box needs the terms of one plane."""
    f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if f.ndim != 4 or f.shape[0] != MOMENT_MODES or g.shape != f.shape:
        raise ValueError(f"moment_record: f[19, nz, ny, nx] and g of the same shape, got {f.shape} and {g.shape}")
    out = np.zeros(MOMENT_WORDS)
    for z in range(f.shape[1]):                            # the planes in sequence, from +0.0
        out = out + plane_profiles(moment_terms(f[:, z:z + 1], g[:, z:z + 1]), (), axis=2)[:, 0]
    return out


def _moment_blocks(sums, who):
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim < 1 or s.shape[-1] != MOMENT_WORDS:
        raise ValueError(f"{who}: sums[..., 95], got shape {s.shape}")
    n = MOMENT_MODES
    return s[..., :n], s[..., n:2 * n], s[..., 2 * n:3 * n], s[..., 3 * n:4 * n], s[..., 4 * n:]


def moment_variances(sums, nsites):
    """(var_f, var_g, var_total)[..., 19] of records sums[..., 95] over boxes of nsites sites: per mode the spatial variance
    sq / n - (sum / n)^2, and the same of the total fluid's moment mf + mg, whose square sum is sq_f + 2 cross + sq_g."""
    sf, sg, qf, qg, x = _moment_blocks(sums, "moment_variances")
    n = float(int(nsites))
    if n < 1:
        raise ValueError(f"moment_variances: nsites >= 1, got {nsites!r}")
    var = lambda s, q: q / n - (s / n) * (s / n)
    return var(sf, qf), var(sg, qg), var(sf + sg, qf + 2. * x + qg)


def equipartition(sums, nsites):
    """(e_f, e_g, e_total)[..., 19]: every mode's variance (moment_variances) over its weight b[a] (MOMENT_NORMS), relative
    to the mean of that ratio over the three momentum modes.  For a thermalised uniform mixture every entry of the
    non-conserved modes is about the same number (1 where the modes share one temperature); rho is conserved at every
    site by the collision and need not be."""
    b = np.array(MOMENT_NORMS)
    out = []
    for v in moment_variances(sums, nsites):
        r = v / b
        out.append(r / r[..., 1:4].mean(axis=-1, keepdims=True))
    return tuple(out)


def stress_series(sums):
    """The box sums of the total fluid's stress moments 4..9, sum_f + sum_g: [..., 6] in the order s_tr, s_xx, s_ww, s_xy,
    s_yz, s_xz.  The off-diagonal ones are the input of a Green-Kubo integral (time_correlation gives the correlation)."""
    sf, sg = _moment_blocks(sums, "stress_series")[:2]
    return sf[..., 4:10] + sg[..., 4:10]


# ---- clusters: the numpy restatement of the cluster trace (include/bflbm.h, "Cluster traces") ----
CLUSTER_WORDS = 38
CLUSTER_CONNECTIVITIES = (6, 26)


def _cluster_occupancy(call, field_zyx, levels, side, connectivity):
    v = np.asarray(field_zyx, dtype=np.float64)
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if v.ndim != 3 or v.size == 0:
        raise ValueError(f"{call}: a field [nz, ny, nx], got shape {v.shape}")
    if v.size > 2 ** 31 - 1:
        raise ValueError(f"{call}: {v.size} sites exceed 2^31 - 1 (labels are 32-bit)")
    if lv.ndim != 1 or not (1 <= len(lv) <= MORPH_MAX_LEVELS):
        raise ValueError(f"{call}: 1..{MORPH_MAX_LEVELS} levels (got shape {lv.shape})")
    if not np.isfinite(lv).all():
        raise ValueError(f"{call}: the levels must be finite (got {lv.tolist()})")
    if side not in MORPH_SIDES and side not in MORPH_SIDES.values():
        raise ValueError(f"{call}: side {side!r}, expected 'above' (0) or 'below' (1)")
    if connectivity not in CLUSTER_CONNECTIVITIES:
        raise ValueError(f"{call}: connectivity must be 6 or 26 (got {connectivity!r})")
    below = bool(MORPH_SIDES.get(side, side))
    with np.errstate(invalid="ignore"):
        return [(v < t) if below else (v >= t) for t in lv]


def _cluster_label_set(occ, connectivity):
    """Canonical labels of a boolean set: every occupied site starts with its own index and takes the minimum over its
    periodic neighbours until nothing changes; between the sweeps a site jumps to its label's label, which is a site of
    its own component with a label no larger, so long chains close in a logarithmic number of sweeps."""
    nz, ny, nx = occ.shape
    none = np.int64(occ.size)
    lab = np.where(occ, np.arange(occ.size, dtype=np.int64).reshape(occ.shape), none)
    offsets = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
               if (dz, dy, dx) != (0, 0, 0) and (connectivity == 26 or abs(dz) + abs(dy) + abs(dx) == 1)]
    while True:
        new = lab
        for d in offsets:
            new = np.minimum(new, np.roll(lab, d, axis=(0, 1, 2)))
        new = np.where(occ, new, none)
        flat = np.append(new.ravel(), none)                # the label of "none" is "none"
        new = np.where(occ, flat[flat[new]], none)         # two jumps
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(occ, lab, -1).astype(np.int32)


def cluster_labels(field_zyx, level, side="above", connectivity=26):
    """labels[nz, ny, nx] int32 of include/bflbm.h, "Cluster traces", in numpy: the smallest linear index
    p = (z ny + y) nx + x of the component of every site with field >= level (side "above" or 0) or field < level (side
    "below" or 1) on the periodic box, -1 where the site is unoccupied; connectivity 6 (faces) or 26 (faces, edges and
    corners).  A NaN occupies nothing on either side."""
    lv = np.asarray(level, dtype=np.float64)
    if lv.ndim != 0:
        raise ValueError(f"cluster_labels: one level (got shape {lv.shape})")
    return _cluster_label_set(_cluster_occupancy("cluster_labels", field_zyx, [float(lv)], side, connectivity)[0], connectivity)


def cluster_sizes(labels):
    """(roots, sizes): the canonical labels that occur in labels[...] (ascending) and how many sites carry each."""
    lab = np.asarray(labels)
    if not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"cluster_sizes: integer labels, got {lab.dtype}")
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    return roots.astype(np.int64), sizes.astype(np.int64)


def cluster_record(field_zyx, levels, side="above", connectivity=26):
    """record[nlevels, 38] int64 of include/bflbm.h, "Cluster traces", in numpy: ncomp, V, smax, the label of the
    largest component (among equals the smallest; -1 if none), the sum of s^2, 0 (capped) and the 32 counts of the
    components with 2^b <= s < 2^(b+1)."""
    out = np.zeros((len(np.atleast_1d(levels)), CLUSTER_WORDS), dtype=np.int64)
    for l, occ in enumerate(_cluster_occupancy("cluster_record", field_zyx, levels, side, connectivity)):
        roots, sizes = cluster_sizes(_cluster_label_set(occ, connectivity))
        out[l, 0], out[l, 1], out[l, 3] = len(roots), sizes.sum(), -1
        if len(roots):
            out[l, 2] = sizes.max()
            out[l, 3] = roots[np.argmax(sizes)]            # the first of the largest: roots ascend
            out[l, 4] = (sizes * sizes).sum()
            out[l, 6:] = np.bincount(np.floor(np.log2(sizes)).astype(np.int64), minlength=32)
    return out


# ---- components: the numpy restatement of the component trace (include/bflbm.h, "Component traces") ----
COMPONENT_HEADER = 6
COMPONENT_ROW = 18
COMPONENT_MAX_ROWS = 256


def component_table(field_zyx, levels, side="above", connectivity=26, min_size=1, rows=COMPONENT_MAX_ROWS):
    """(header[nlevels, 6], table[nlevels, rows, 18]) int64 of include/bflbm.h, "Component traces", in numpy.  Header:
    ncomp, V, nqual, Vqual, nrows, 0 (capped).  Row j, the qualifying component (size >= min_size) with j qualifying
    components of smaller label: label, size, origin (x, y, z), extent, sum d, sum d^2, sum dx dy, dx dz, dy dz, faces,
    with d = (c - origin) mod n; unused rows have label -1 and zeros elsewhere."""
    occs = _cluster_occupancy("component_table", field_zyx, levels, side, connectivity)
    _component_refuse("component_table", min_size, rows)
    parts = [component_table_from_labels(_cluster_label_set(occ, connectivity), min_size, rows) for occ in occs]
    return np.stack([h for h, _ in parts]), np.stack([t for _, t in parts])


def _component_refuse(call, min_size, rows):
    if int(min_size) != min_size or min_size < 1:
        raise ValueError(f"{call}: min_size must be an integer >= 1 (got {min_size!r})")
    if int(rows) != rows or not (1 <= rows <= COMPONENT_MAX_ROWS):
        raise ValueError(f"{call}: rows must be in 1..{COMPONENT_MAX_ROWS} (got {rows!r})")


def component_table_from_labels(labels_zyx, min_size=1, rows=COMPONENT_MAX_ROWS):
    """(header[6], table[rows, 18]) int64 of one level from canonical labels[nz, ny, nx] (cluster_labels, or one replica
    of ClusterTrace.labels()): what component_table makes of every level."""
    lab = np.asarray(labels_zyx)
    if lab.ndim != 3 or lab.size == 0 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"component_table_from_labels: integer labels [nz, ny, nx], got shape {lab.shape} of {lab.dtype}")
    _component_refuse("component_table_from_labels", min_size, rows)
    min_size, rows = int(min_size), int(rows)
    nz, ny, nx = lab.shape
    n = (nx, ny, nz)
    occ = lab >= 0
    header = np.zeros(COMPONENT_HEADER, dtype=np.int64)
    t = np.zeros((rows, COMPONENT_ROW), dtype=np.int64)
    t[:, 0] = -1
    roots, sizes = cluster_sizes(lab)
    qual = sizes >= min_size
    nrows = min(int(qual.sum()), rows)
    header[:] = (len(roots), sizes.sum(), qual.sum(), sizes[qual].sum(), nrows, 0)
    if nrows == 0:
        return header, t
    kept = roots[qual][:nrows]
    t[:nrows, 0], t[:nrows, 1] = kept, sizes[qual][:nrows]
    p = np.flatnonzero(occ.ravel())
    slot = np.searchsorted(kept, lab.ravel()[p])
    inside = (slot < nrows) & (kept[np.minimum(slot, nrows - 1)] == lab.ravel()[p])
    p, slot = p[inside], slot[inside]
    c = (p % nx, (p // nx) % ny, p // (nx * ny))           # x, y, z
    bare = sum((~np.roll(occ, s, axis=a)).astype(np.int64) for a in range(3) for s in (1, -1))   # unoccupied periodic neighbours
    d = []
    for a in range(3):
        present = np.zeros((nrows, n[a]), dtype=bool)
        present[slot, c[a]] = True
        starts = present & ~np.roll(present, 1, axis=1)    # the predecessor is unoccupied
        origin = np.where(starts.any(axis=1), starts.argmax(axis=1), 0).astype(np.int64)
        t[:nrows, 2 + a], t[:nrows, 5 + a] = origin, present.sum(axis=1)
        d.append((c[a] - origin[slot]) % n[a])
    sums = list(d) + [v * v for v in d] + [d[0] * d[1], d[0] * d[2], d[1] * d[2], bare.ravel()[p]]
    for w, v in enumerate(sums):
        np.add.at(t[:, 8 + w], slot, v)                    # integer adds: exact
    return header, t


def component_centroids(table, n):
    """[..., 3]: the centroids (x, y, z) in cell indices of table[..., 18] on the box n = (nx, ny, nz),
    (origin + sum d / size) mod n; NaN along a spanned axis (extent == n: no unwrapping exists) and in unused rows."""
    t = np.asarray(table)
    n = np.asarray(n, dtype=np.float64)
    size = t[..., 1:2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.mod(t[..., 2:5] + t[..., 8:11] / size, n)
    return np.where((t[..., 0:1] >= 0) & (t[..., 5:8] < n), c, np.nan)


def component_gyration(table):
    """[..., 3, 3] float64: the central second-moment tensor sum d_a d_b / size - (sum d_a / size)(sum d_b / size) of
    table[..., 18], axes x, y, z; NaN in unused rows.  Along a spanned axis it is taken about coordinate 0."""
    t = np.asarray(table)
    size = np.where(t[..., 0] >= 0, t[..., 1], 0).astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = t[..., 8:11] / size
        d2, cross = t[..., 11:14] / size, t[..., 14:17] / size
    g = np.empty(t.shape[:-1] + (3, 3))
    for a in range(3):
        g[..., a, a] = d2[..., a]
    for k, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        g[..., a, b] = g[..., b, a] = cross[..., k]
    return g - m1[..., :, None] * m1[..., None, :]


def track_components(centroids, sizes, n, max_jump):
    """Unwrapped trajectories [ntracks, T, 3] from the rows of consecutive samples: centroids[T, R, 3] (NaN: no
    position) and sizes[T, R] (0: unused row) of one replica and level on the periodic box n = (nx, ny, nz).  A
    component's label, and with it its row, changes whenever it drifts across the box origin, so rows are linked by
    position: between consecutive samples the pairs (track, row) within max_jump of each other by the minimum image are
    taken greedily by ascending distance, ties by the smaller track, then the smaller row.  A row left over starts a new
    track, a track left over ends.  NaN before birth and after loss: ready for msd per track."""
    c = np.asarray(centroids, dtype=np.float64)
    s = np.asarray(sizes)
    n = np.asarray(n, dtype=np.float64)
    if c.ndim != 3 or c.shape[-1] != 3 or s.shape != c.shape[:2]:
        raise ValueError(f"track_components: centroids[T, R, 3] and sizes[T, R], got {c.shape} and {s.shape}")
    if not max_jump > 0:
        raise ValueError(f"track_components: max_jump must be > 0 (got {max_jump!r})")
    steps = c.shape[0]
    tracks, live = [], {}                                  # live: track index -> (wrapped, unwrapped) position
    for t in range(steps):
        rows = [r for r in range(c.shape[1]) if s[t, r] > 0 and np.isfinite(c[t, r]).all()]
        pairs = []
        for k, (wrapped, _) in live.items():
            for r in rows:
                step = np.mod(c[t, r] - wrapped + 0.5 * n, n) - 0.5 * n
                dist = float(np.sqrt((step * step).sum()))
                if dist <= max_jump:
                    pairs.append((dist, k, r, step))
        taken, new_live = set(), {}
        for dist, k, r, step in sorted(pairs, key=lambda q: q[:3]):
            if k in new_live or r in taken:
                continue
            taken.add(r)
            new_live[k] = (c[t, r], live[k][1] + step)
        for r in rows:
            if r not in taken:
                tracks.append(np.full((steps, 3), np.nan))
                new_live[len(tracks) - 1] = (c[t, r], c[t, r].copy())
        live = new_live
        for k, (_, unwrapped) in live.items():
            tracks[k][t] = unwrapped
    return np.array(tracks).reshape(len(tracks), steps, 3)


PRESSURE_VARIABLES = ["rho", "phi", "afx", "afy", "afz", "agx", "agy", "agz"]
PRESSURE_PAIRS = [("rho", "phi"), ("afx", "agx"), ("afy", "agy"), ("afz", "agz")]


def pressure_profile_inputs():
    """(variables, pairs) a profile trace must record for pressure_profile: the 8 hydrovs variables rho, phi, af*, ag*
    and the 4 pairs rho phi, afx agx, afy agy, afz agz, by name."""
    return list(PRESSURE_VARIABLES), list(PRESSURE_PAIRS)


def pressure_profile(means, names, alpha0, cs2=1.0 / 3.0, axis=2, pairs=None):
    """The static part of the pressure tensor of Surface_Tension.ipynb (cell 2) with G = alpha0, from plane means
    [..., Q, n_a] of a profile trace along `axis` (the normal) whose variables are `names` and whose pairs are `pairs`
    ((a, b) of names or slots; None: those of pressure_profile_inputs, in that order):
        p_bulk      = cs2 (<rho> + <phi>) + alpha0 cs2 <rho phi>
        pn_minus_pt = -( <af_n ag_n> - 1/2 (<af_t1 ag_t1> + <af_t2 ag_t2>) ) / alpha0
    with af = -cs2 alpha0 grad phi, ag = -cs2 alpha0 grad rho, so that pn_minus_pt = -alpha0 cs2^2 (d_n rho d_n phi -
    1/2 sum_t d_t rho d_t phi).  The kinetic rho u u part is not included.  Returns (p_bulk, pn_minus_pt), each
    [..., n_a]."""
    m = np.asarray(means, dtype=np.float64)
    axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
    if axis not in (0, 1, 2):
        raise ValueError(f"pressure_profile: axis {axis!r}, expected 0..2")
    if alpha0 == 0:
        raise ValueError("pressure_profile: alpha0 == 0 (no interaction: the tensor has no gradient part)")
    names = list(names)
    pairs = list(PRESSURE_PAIRS if pairs is None else pairs)
    if m.ndim < 2 or m.shape[-2] != len(names) + len(pairs):
        raise ValueError(f"pressure_profile: means[..., Q, n_a] with Q = {len(names)} variables + {len(pairs)} pairs, got {m.shape}")

    def slot(v):
        if not isinstance(v, str):
            return int(v)
        if v not in names:
            raise ValueError(f"pressure_profile: the mean of {v!r} is missing (recorded: {names})")
        return names.index(v)

    have = {tuple(sorted((slot(a), slot(b)))): len(names) + k for k, (a, b) in enumerate(pairs)}

    def mean_of(a, b=None):
        if b is None:
            return m[..., slot(a), :]
        key = tuple(sorted((slot(a), slot(b))))
        if key not in have:
            raise ValueError(f"pressure_profile: the mean of {a} {b} is missing (recorded pairs: {pairs})")
        return m[..., have[key], :]

    d = "xyz"
    n, t1, t2 = d[axis], d[(axis + 1) % 3], d[(axis + 2) % 3]
    p_bulk = cs2 * (mean_of("rho") + mean_of("phi")) + alpha0 * cs2 * mean_of("rho", "phi")
    pn_minus_pt = -(mean_of("af" + n, "ag" + n) - 0.5 * (mean_of("af" + t1, "ag" + t1) + mean_of("af" + t2, "ag" + t2))) / alpha0
    return p_bulk, pn_minus_pt


def mechanical_surface_tension(pn_minus_pt, interfaces=2):
    """gamma = integral (P_N - P_T) dn as the plain sum over the last axis (lattice spacing 1), divided by the number of
    interfaces the periodic box holds (2 for a stripe)."""
    return np.asarray(pn_minus_pt, dtype=np.float64).sum(axis=-1) / float(interfaces)


# ---- radial shells: the numpy restatement of the radial trace (include/bflbm.h, "Radial traces") and the droplet route to
# the surface tension of Surface_Tension.ipynb (pressure inside and outside, the Shan-Chen force integral, a radius) ----
RADIAL_TILE, RADIAL_MAX_BINS = 256, 128                     # the sites of a tile; the most shells


def _radial_slots(nv, pairs, radials, who):
    pairs = [(int(a), int(b)) for a, b in pairs]
    rads = [(-1 if w is None else int(w), tuple(int(c) for c in v)) for w, v in radials]
    if any(not (0 <= a < nv and 0 <= b < nv) for a, b in pairs):
        raise ValueError(f"{who}: a pair slot outside the {nv} variables: {pairs}")
    if any(not (-1 <= w < nv) or len(v) != 3 or any(not (0 <= c < nv) for c in v) for w, v in rads):
        raise ValueError(f"{who}: a radial term (w, (vx, vy, vz)) with a slot outside the {nv} variables (w = -1 or None: none): {rads}")
    return pairs, rads


def radial_shells(fields, centre, delta, nbins, pairs=(), radials=()):
    """(counts[nbins], sums[Q, nbins]) of include/bflbm.h, "Radial traces", in numpy, operation for operation and in the
    header's order: fields[nvars, nz, ny, nx], centre (cx, cy, cz) in cell indices (a NaN puts every site in no shell),
    shells of width delta, pairs a list of (a, b) variable slots, radials a list of (w, (vx, vy, vz)) variable slots with
    w = None or -1 for the bare projection.  Q = nvars + pairs + radials.  An unbuffered np.add.at over the members of a
    tile adds them sequentially in index order, which is the order of the definition."""
    x = np.asarray(fields, dtype=np.float64)
    c = np.asarray(centre, dtype=np.float64)
    delta, nbins = float(delta), int(nbins)
    if x.ndim != 4 or c.shape != (3,):
        raise ValueError(f"radial_shells: fields[nvars, nz, ny, nx] and a centre of 3, got {x.shape} and {c.shape}")
    if not (np.isfinite(delta) and delta > 0) or not (1 <= nbins <= RADIAL_MAX_BINS):
        raise ValueError(f"radial_shells: delta finite and > 0, nbins in 1..{RADIAL_MAX_BINS}, got {delta} and {nbins}")
    nv, nz, ny, nx = x.shape
    pairs, rads = _radial_slots(nv, pairs, radials, "radial_shells")
    d = []
    for a, n in enumerate((nx, ny, nz)):                   # the minimum image, per axis
        da = np.arange(n, dtype=np.float64) - c[a]
        h = 0.5 * float(n)
        da = np.where(da >= h, da - float(n), np.where(da < -h, da + float(n), da))
        d.append(da)
    dx, dy, dz = d[0][None, None, :], d[1][None, :, None], d[2][:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        q = r / delta
        member = q < float(nbins)                          # false for a NaN
        shell = np.where(member, q, 0.0).astype(np.int64)
        terms = [np.ones_like(r)] + [x[v] for v in range(nv)] + [x[a] * x[b] for a, b in pairs]
        for w, (vx, vy, vz) in rads:
            p = ((x[vx] * dx + x[vy] * dy) + x[vz] * dz) / r
            p = np.where(r == 0, 0.0, p)
            terms.append(p if w < 0 else x[w] * p)
    terms = np.stack(terms).reshape(len(terms), nz, ny * nx)
    member, shell = member.reshape(nz, ny * nx), shell.reshape(nz, ny * nx)
    total = np.zeros((len(terms), nbins))
    for z in range(nz):                                    # the planes in sequence
        plane = np.zeros((len(terms), nbins))
        for t0 in range(0, ny * nx, RADIAL_TILE):          # the tiles in order
            sel = np.nonzero(member[z, t0:t0 + RADIAL_TILE])[0] + t0
            part = np.zeros((len(terms), nbins))
            for k in range(len(terms)):
                np.add.at(part[k], shell[z, sel], terms[k, z, sel])
            plane = plane + part
        total = total + plane
    return total[0], total[1:]


RADIAL_VARIABLES = ["rho", "phi", "afx", "afy", "afz", "agx", "agy", "agz"]
RADIAL_PAIRS = [("rho", "phi")]
RADIAL_RADIALS = [("rho", ("afx", "afy", "afz")), ("phi", ("agx", "agy", "agz"))]


def laplace_inputs():
    """(variables, pairs, radials) a radial trace must record for the droplet route to the surface tension: the 8 hydrovs
    variables rho, phi, af*, ag*, the pair rho phi and the radial terms rho (af . r^) and phi (ag . r^), by name."""
    return list(RADIAL_VARIABLES), list(RADIAL_PAIRS), list(RADIAL_RADIALS)


def _radial_row(means, names, who, a, b=None, npairs=len(RADIAL_PAIRS)):
    """The shell means of variable a, of the pair (a, b) or of the radial term a = ("rad", k), from means[..., Q, nbins] laid
    out as laplace_inputs() asks."""
    names = list(names)
    for v in (a, b):
        if isinstance(v, str) and v not in names:
            raise ValueError(f"{who}: the mean of {v!r} is missing (recorded: {names})")
    if isinstance(a, tuple):
        return means[..., len(names) + npairs + a[1], :]
    if b is None:
        return means[..., names.index(a), :]
    k = [tuple(sorted(p)) for p in RADIAL_PAIRS].index(tuple(sorted((a, b))))
    return means[..., len(names) + k, :]


def radial_pressure(means, names, alpha0, cs2=1.0 / 3.0):
    """p(r) = cs2 (<rho> + <phi>) + alpha0 cs2 <rho phi> per shell, [..., nbins], from the shell means [..., Q, nbins] of a
    radial trace recorded with laplace_inputs() (`names`: its variables): the bulk pressure of Surface_Tension.ipynb
    (cell 13: p = rhot cs2 + alpha0 cs2 rho phi) with the product averaged before it is multiplied."""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim < 2 or m.shape[-2] != len(names) + len(RADIAL_PAIRS) + len(RADIAL_RADIALS):
        raise ValueError(f"radial_pressure: means[..., Q, nbins] with Q = {len(names)} variables + {len(RADIAL_PAIRS)} pair + "
                         f"{len(RADIAL_RADIALS)} radial terms, got {m.shape}")
    rho, phi = _radial_row(m, names, "radial_pressure", "rho"), _radial_row(m, names, "radial_pressure", "phi")
    return cs2 * (rho + phi) + alpha0 * cs2 * _radial_row(m, names, "radial_pressure", "rho", "phi")


def _shell_mean(v, counts, sel):
    w = np.where(sel, np.asarray(counts, dtype=np.float64), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w > 0, np.nan_to_num(v) * w, 0.0).sum(axis=-1) / w.sum(axis=-1)


def pressure_jump(p, counts, r, r_in, r_out):
    """Delta p = (count-weighted mean of p over the shells with r < r_in) - (that over the shells with r >= r_out): the
    inside minus the outside pressure of the Laplace law.  p, counts [..., nbins]; r [nbins] the shell radii; NaN where
    either side holds no site."""
    r = np.asarray(r, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    return _shell_mean(p, counts, r < r_in) - _shell_mean(p, counts, r >= r_out)


def radial_force_integral(means, names, delta, n):
    """The Shan-Chen force integrated from the edge of the box to the droplet's centre, in box units: the shell form of
    Surface_Tension.ipynb's  sum_ix (rho afx + phi agx)[ix, nc, nc] dr,  ix = 0 .. n/2 - 1, dr = 1 / n  (cell 13;
    tests/test_gpu_notebook_surface_tension.py, _check_system: force_rho + force_phi, compared with deltaP_SC).  The
    notebook walks along +x from the edge at ix = 0 towards the centre at ix = nc, that is against the outward radial
    unit vector r^, so its integrand is -(rho af + phi ag) . r^: the result here is
        - sum over the shells with r = (k + 1/2) delta < n / 2 of (<rho af . r^> + <phi ag . r^>) delta / n
    and carries the notebook's sign (positive for a droplet, about Delta p).  means [..., Q, nbins] as radial_pressure
    takes them; n: the box extent along the notebook's line (the smallest extent of a box that is no cube)."""
    m = np.asarray(means, dtype=np.float64)
    nbins = m.shape[-1]
    inside = (np.arange(nbins) + 0.5) * float(delta) < 0.5 * float(n)
    f = _radial_row(m, names, "radial_force_integral", ("rad", 0)) + _radial_row(m, names, "radial_force_integral", ("rad", 1))
    return -(np.where(inside, np.nan_to_num(f), 0.0).sum(axis=-1)) * float(delta) / float(n)


def fit_radial_profile(r, rho_mean, counts):
    """Count-weighted least-squares fit of rho(r) = hi - (hi - lo) / 2 (1 + tanh((r - R) / W)) to the shell means
    rho_mean[nbins] at the radii r[nbins] (every shell stands for `counts` sites; empty shells are left out); returns
    (hi, lo, R, W) in the units of r.  The 1-D stand-in for fit_droplet on a radial trace's record."""
    from scipy.optimize import curve_fit

    def profile(r, hi, lo, radius, width):
        return hi - (hi - lo) / 2 * (1 + np.tanh((r - radius) / width))

    r, rho, w = (np.asarray(v, dtype=np.float64) for v in (r, rho_mean, counts))
    keep = w > 0
    r, rho, w = r[keep], rho[keep], w[keep]
    half = r[np.argmin(np.abs(rho - 0.5 * (rho[0] + rho[-1])))]           # start: the shell nearest to half height, one shell wide
    p0 = [rho[0], rho[-1], half, float(r[1] - r[0]) if len(r) > 1 else 1.0]
    popt, _ = curve_fit(profile, r, rho, p0=p0, sigma=1.0 / np.sqrt(w))
    return tuple(popt)


def equimolar_radius(rho_mean, counts):
    """The radius R_e of the sphere that holds the droplet's excess mass at the inner density:
    4/3 pi R_e^3 (hi - lo) = sum_k counts_k (rho_k - lo), hi and lo the means of the innermost and the outermost
    non-empty shell.  In cells (a shell's sites count its volume), whatever delta is; no transcendental function."""
    rho, w = np.asarray(rho_mean, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    keep = w > 0
    rho, w = rho[keep], w[keep]
    hi, lo = rho[0], rho[-1]
    return float((3.0 * (w * (rho - lo)).sum() / (4.0 * np.pi * (hi - lo))) ** (1.0 / 3.0))


def com_from_moments(m, n, weighted=False):
    """Centre of mass in unit-box cell-centre coordinates; weighted=True is the reference's C++ getCenterOfMass
    (trapezoid weights, LBM_hydrovs.H:62-113), False the notebooks' plain sum."""
    o = 10 if weighted else 0
    return np.array([(m[o + 1 + d] / m[o] + 0.5) / n[d] for d in range(3)])


def covariance_from_moments(m, n, kind="notebook"):
    """Second central mass moments. kind="notebook": trapezoid-weighted sums about the unweighted COM,
    normalised by the weighted mass (mass_covariance above); kind="reference": plain sums about the
    trapezoid-weighted COM, normalised by the plain mass (fittingDropletCovariance, LBM_hydrovs.H:262-335)."""
    if kind == "notebook":
        r0, o = com_from_moments(m, n, False), 10
    else:
        r0, o = com_from_moments(m, n, True), 0
    s0 = m[o]
    s1 = np.array([(m[o + 1 + d] + 0.5 * s0) / n[d] for d in range(3)])          # sum w (i+1/2)/n
    idx = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}
    c = np.empty((3, 3))
    for (a, b), k in idx.items():
        # sum w (i+1/2)(j+1/2) = S_ab + (S_a + S_b)/2 + S_0/4
        s2 = (m[o + k] + 0.5 * (m[o + 1 + a] + m[o + 1 + b]) + 0.25 * s0) / (n[a] * n[b])
        c[a, b] = c[b, a] = (s2 - r0[a] * s1[b] - r0[b] * s1[a] + r0[a] * r0[b] * s0) / s0
    return c


def principal_axes_from_moments(m, n, radius, kind="notebook"):
    ev, vec = np.linalg.eig(covariance_from_moments(m, n, kind))
    axes = np.array([ev[k] ** (1. / 3.) * radius / (ev[(k + 1) % 3] * ev[(k + 2) % 3]) ** (1. / 6.) for k in range(3)])
    return axes, ev, vec
