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
