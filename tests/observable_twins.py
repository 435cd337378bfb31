"""Host twins and comparisons that several GPU test files share: the numpy twin of the reference's gradient-flow radius
fit (tests/test_gpu_droplet.py, tests/test_gpu_wide_planes.py) and the exact comparison of interface heights
(tests/test_gpu_iface.py, tests/test_gpu_wide_planes.py).  Test infrastructure only."""
import numpy as np


def same_doubles(a, b):
    """Equal doubles, NaNs matched by position."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def flow_twin(pkg, rho, W0, R0, nstep, window, eta=0.2, dt=0.02):
    """Host twin of fittingDroplet (LBM_hydrovs.H:117-148): the two lattice integrals with numpy, the closed forms from
    the library's host function (tests/test_flowfit.py checks those against quadrature)."""
    import ctypes
    lib = pkg._lib.load()
    nz, ny, nx = rho.shape
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    m = rho.sum()
    r0 = np.array([(rho * x).sum(), (rho * y).sum(), (rho * z).sum()]) / m
    rr = np.sqrt((x - r0[0]) ** 2 + (y - r0[1]) ** 2 + (z - r0[2]) ** 2)
    C0 = rho.max() - rho.min()
    cell = 1.0 / rho.size
    W, R, traj = W0, R0, [(W0, R0)]
    out = (ctypes.c_double * 9)()
    for _ in range(1, nstep):
        assert lib.bflbm_flowfit_coefficients(W, R, eta, eta, dt, C0, out) == 0
        Jrr, Jwr, Jrw, Jww, Kw, Kr = list(out)[:6]
        s = np.sqrt(2 * W)
        dist = R - rr
        sech2 = 1.0 / np.cosh(dist / s) ** 2
        MfW = (rho * dist * sech2).sum() * cell / s ** 3
        MfR = (rho * sech2).sum() * cell / s
        C = (MfW - 0.5 * Kw, MfR - 0.5 * Kr)
        det = (1 - Jww) * (1 - Jrr) - Jwr * Jrw
        dW = ((1 - Jrr) * (-eta * dt) * C[0] + Jwr * (eta * dt) * C[1]) / det
        dR = (Jrw * (-eta * dt) * C[0] + (1 - Jww) * (eta * dt) * C[1]) / det
        W += dW; R += dR
        if W <= 0:
            W -= dW; dt /= 5
        if abs(W) < 1e-6:
            W = W0
        traj.append((W, R))
    t = np.array(traj[-window:])
    return t.mean(axis=0), (t.max(axis=0) - t.min(axis=0)) / t.mean(axis=0)
