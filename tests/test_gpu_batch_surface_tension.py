"""GPU: the nine Surface_Tension.ipynb systems as ONE replica batch -- nine 32^3 droplets, two parameter sets
(alpha0 = 1.5 / kappa = 0.1 and alpha0 = 1.7 / kappa = 1.0, rho_hi = 3), per-replica radii, 20000 steps -- held to the
notebook's printed numbers and Laplace-law surface tensions with the tolerances and tables of
tests/test_gpu_notebook_surface_tension.py (which runs the same nine systems one lattice after another)."""
import time

import numpy as np
import pytest

import test_gpu_notebook_surface_tension as nb

pytestmark = pytest.mark.gpu

SETS = [(1.5, 0.1, 16, nb.CELL13, nb.R_15, nb.GAMMA_15), (1.7, 1.0, 15, nb.CELL18, nb.R_17, nb.GAMMA_17)]


def test_nine_droplets_as_one_batch(pkg):
    params, radii = [], []
    for alpha0, kappa, _, systems, _, _ in SETS:
        for rec in systems:
            params.append(dict(rho_hi=3.0, alpha0=alpha0, kappa=kappa))
            radii.append(rec[0])
    t0 = time.perf_counter()
    with pkg.BatchLBM(nb.N, params=params) as b:
        for rep, r in zip(b.replicas, radii):
            rep.LBM_init_droplet(r)
        b.LBM_timestep(20000)
        b.sync()
        t_steps = time.perf_counter() - t0
        h = b.LBM_hydrovars()
        fits = [rep.fit_droplet()[2] for rep in b.replicas]
        schedule = b.resolved_schedule()
    print(f"\nnine 32^3 droplets, one batch ({schedule}): 20000 steps in {t_steps:.2f} s")
    k0 = 0
    for alpha0, kappa, nc, systems, nb_radii, gamma in SETS:
        dps = []
        for j, rec in enumerate(systems):
            fields = {k: np.ascontiguousarray(h[k0 + j, c].transpose(2, 1, 0))
                      for k, c in dict(rho=0, phi=1, rhot=5, afx=9, agx=12).items()}
            dps.append(nb._check_system(fields, alpha0, nc, rec))
        k, b0 = nb._regression(nb_radii, dps)
        assert abs(k - gamma[0]) <= 1e-9 * gamma[0] and abs(b0 - gamma[1]) <= 1e-8 * gamma[1], (k, b0)
        assert abs(k / 2 - gamma[2]) <= 1e-9 * gamma[2]
        np.testing.assert_allclose(fits[k0:k0 + len(systems)], nb_radii, rtol=2e-6)
        k0 += len(systems)
