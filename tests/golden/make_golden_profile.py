#!/usr/bin/env python3
"""Writes tests/golden/profile_stripe.npz: the profile-trace record of a flat stripe from the CPU oracle, the fixture
of tests/test_gpu_profile.py::test_stripe_pressure_profile_gives_the_mechanical_surface_tension.

An 8 x 8 x 64 stripe (frac = 0.5, rho_hi = 3, rho_lo = 0, tau = 1/2, kBT = 0) run for 20000 steps at
(alpha0, kappa) = (1.5, 0.1) and (1.7, 1.0), the two parameter sets of Surface_Tension.ipynb's Laplace fits.  Stored per
case: the plane sums along z of the pressure variables (analysis.pressure_profile_inputs: 8 hydrovs variables and 4
pairs), formed from the oracle's hydrovs in the order of include/bflbm.h, "Profile traces", by tests/profile_sums.emulate:
  sums/<case>    float64 [12, 64]
  gamma/<case>   the mechanical surface tension 1/2 sum_z (P_N - P_T)(z) of that record (analysis.pressure_profile)
NOT reference outputs (the reference cannot be built here): they freeze the CPU oracle (oracle/bflbm_oracle.c, gcc -O3
-ffp-contract=off).  Two to three minutes of CPU.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import oracle_binding as ob  # noqa: E402
import profile_sums as ps  # noqa: E402

PATH = os.path.join(HERE, "profile_stripe.npz")
SHAPE = (8, 8, 64)
STEPS = 20000
CASES = {"a15_k01": dict(alpha0=1.5, kappa=0.1), "a17_k10": dict(alpha0=1.7, kappa=1.0)}
COMMON = dict(rho_hi=3.0, rho_lo=0.0, tau_f=0.5, tau_g=0.5, kBT=0.0)
VARIABLES = "rho phi afx afy afz agx agy agz".split()
PAIRS = [("rho", "phi"), ("afx", "agx"), ("afy", "agy"), ("afz", "agz")]
HYDROVS = ["rho", "phi", "ufx", "ufy", "ufz", "p_bulk", "ugx", "ugy", "ugz", "afx", "afy", "afz", "agx", "agy", "agz"]


def _analysis():
    """analysis.py alone: it needs numpy only, not the HIP library."""
    spec = importlib.util.spec_from_file_location("bflbm_analysis", os.path.join(os.path.dirname(TESTS), "binary-fluctuating-lattice-boltzmann_amd", "analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load():
    return {k.replace("__", "/"): v for k, v in np.load(PATH).items()}


def build():
    an = _analysis()
    out = {}
    for name, par in CASES.items():
        ref = ob.OracleLattice(*SHAPE, params=ob.default_params(**COMMON, **par))
        ref.init_stripe(0.5)
        for _ in range(STEPS):
            ref.timestep()
        fields = ref.h[[HYDROVS.index(v) for v in VARIABLES]]
        slots = [(VARIABLES.index(a), VARIABLES.index(b)) for a, b in PAIRS]
        sums = ps.emulate(fields, slots, "z")
        assert np.array_equal(sums, an.plane_profiles(fields, slots, "z"))
        pnt = an.pressure_profile(sums / float(SHAPE[0] * SHAPE[1]), VARIABLES, par["alpha0"], ref.p.cs2, "z")[1]
        out[f"sums/{name}"] = sums
        out[f"gamma/{name}"] = np.float64(an.mechanical_surface_tension(pnt, interfaces=2))
        print(name, "gamma_mech = %.11f, largest |u_f| = %.3g" % (out[f"gamma/{name}"], np.abs(ref.h[2:5]).max()))
    out["steps"] = np.int64(STEPS)
    out["shape"] = np.array(SHAPE, dtype=np.int64)
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **{k.replace("/", "__"): v for k, v in build().items()})
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
