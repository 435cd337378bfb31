#!/usr/bin/env python3
"""Writes tests/golden/reference_*.npz: output of the REFERENCE's own compiled code (oracle/_ref/ref_main: LBM_d3q19.H and
LBM_binary.H compiled unmodified against oracle/ref_harness/amrex_lite.H).  Unlike the oracle_*.npz files beside them
these are not oracle output; the oracle is used here only to make INPUT data (uploaded states, the project's own
stream of normals).  Runs only where oracle/_ref/ exists (the reference's headers are needed to build it).

Every file carries `meta`: a JSON text with the compiler, the flags and, per case, lattice, parameters, init and steps.
Keys are "<case>/<step>/<name>" with name in f, g, hbar (15 comps), h (22), fn, gn, and "<case>/f0", "<case>/g0" for
uploaded states.  An entry of dtype uint8 is the SHA-256 of the little-endian bytes of `x + 0.0` (as in
oracle_golden_v2.npz); small lattices carry full arrays.

  reference_trajectories.npz   kBT = 0: steps {0, 1, 3, 10} on ragged and degenerate boxes, the three inits and uploaded
                               states, tau on both sides of the unit-rate dispatch, alpha0 x (rho_hi + rho_lo) <= 6
  reference_noise_injected.npz kBT > 0 with the noise of EVERY step recorded (normals from a seeded numpy table), so that
                               the project side can inject it
  reference_noise_generated.npz  the table is the project's own stream in the reference's call order, so that the
                               project's generated noise can be compared: densities and the reference's noise field
  reference_tiling.npz         65 x 9 x 3 (an exact-schedule tile edge, digests) and 64 x 8 x 9 (hand-over schedule)
  reference_units.npz          the six site functions on seeded random inputs; thermal_noise of the USE_REF_STATE build
                               for shifts of zero, negative, beyond half the box and just inside one box length
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_v2 import digest  # noqa: E402

FULL_ARRAYS_UP_TO = 64            # sites; larger lattices carry digests
STEPS = (0, 1, 3, 10)
ONE_ULP_ABOVE = float(np.nextafter(0.5, 1.0))
SEED = 12345                      # the project's default seed (LBM_binary.H:17)
W = np.array([1 / 3] + [1 / 18] * 6 + [1 / 36] * 12)


def path(name):
    return os.path.join(HERE, f"reference_{name}.npz")


def load(name):
    z = {k.replace("__", "/"): v for k, v in np.load(path(name)).items()}
    meta = json.loads(str(z.pop("meta")))
    return meta, z


def other_rate(direction):
    from test_unit_rate_premise import nearest_tau_with_another_rate
    return nearest_tau_with_another_rate(direction)


# ---- inputs made on the project side -------------------------------------------------------------------------------

def upload_state(n, spec):
    """("oracle_droplet", r, rho_lo, rho_hi, kappa): the droplet profile at another density range than the reference's
    compile-time rho_lo / rho_hi (LBM_binary.H:25-26), which only its own inits read; ("random", seed, lo_f, lo_g): an
    asymmetric random state; ("signed", seed): random densities of both signs and exact zeros, at rest."""
    import oracle_binding as ob
    nx, ny, nz = n
    if spec[0] == "oracle_droplet":
        _, r, lo, hi, kappa = spec
        o = ob.OracleLattice(nx, ny, nz, ob.default_params(rho_lo=lo, rho_hi=hi, kappa=kappa))
        o.init_droplet(r)
        return o.f.copy(), o.g.copy()
    rng = np.random.default_rng(spec[1])
    shp = (19, nz, ny, nx)
    if spec[0] == "random":
        return (W[:, None, None, None] * (spec[2] + 0.2 * rng.random(shp)), W[:, None, None, None] * (spec[3] + 0.2 * rng.random(shp)))
    minority = rng.uniform(-0.3, 0.3, shp[1:])                 # one fluid near zero, of either sign ...
    minority.flat[::7] = 0.0                                  # ... or exactly zero
    majority = rng.uniform(0.8, 1.2, shp[1:])                  # the other keeps rho + phi >= 0.5: no 0/0 in the reference
    f_is_minority = rng.random(shp[1:]) < 0.5
    rho = np.where(f_is_minority, minority, majority)
    phi = np.where(f_is_minority, majority, minority)
    return W[:, None, None, None] * rho, W[:, None, None, None] * phi


def project_normals(n, steps, seed=SEED):
    """The project's own stream for noise indices 0..steps, every site in z, y, x order, in the reference's call order."""
    import oracle_binding as ob
    import reference_binding as rb
    ns = n[0] * n[1] * n[2]
    tab = np.empty((steps + 1, ns, 33))
    for t in range(steps + 1):
        for s in range(ns):
            tab[t, s] = ob.site_normals(seed, s, t)
    return rb.reference_order(tab)


def ref_fields(n, seed, signed=False):
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    rho = (-0.2 if signed else 0.2) + rng.random((nz, ny, nx))
    phi = (-0.1 if signed else 0.1) + rng.random((nz, ny, nx))
    rhot = rho + phi + 0.01 * rng.random((nz, ny, nx))
    return rho, phi, rhot


# ---- the cases -----------------------------------------------------------------------------------------------------

def trajectory_cases():
    lo, hi = other_rate(0.0), other_rate(1.0)
    nb1 = ("upload", ("oracle_droplet", 0.3, 0.1, 3.0, 0.1))       # Surface_Tension.ipynb: alpha0 = 1.5, kappa = 0.1, rho_hi = 3
    nb2 = ("upload", ("oracle_droplet", 0.275, 0.1, 3.0, 1.0))     #                         alpha0 = 1.7, kappa = 1
    c = [
        ("stripe8", (8, 8, 8), ("stripe", 0.5), dict()),                                          # SURVEY 8c's case
        ("mixture8", (8, 8, 8), ("mixture",), dict(tau_f=1.0, tau_g=1.0, alpha0=0.0, kappa=1.0)),
        ("stripe8_tau1", (8, 8, 8), ("stripe", 0.5), dict(tau_f=1.0, tau_g=1.0, alpha0=2.5)),
        ("notebook8", (8, 8, 8), nb2, dict(alpha0=1.7, kappa=1.0)),
        ("droplet10", (10, 6, 13), ("droplet", 0.3), dict()),
        ("notebook10", (10, 6, 13), nb1, dict(alpha0=1.5, kappa=0.1)),
        ("stripe10_tau", (10, 6, 13), ("stripe", 0.5), dict(tau_f=0.8, tau_g=0.6)),
        ("droplet7_tau", (7, 9, 5), ("droplet", 0.3), dict(tau_f=0.8, tau_g=0.6, alpha0=1.5, kappa=0.1)),
        ("random7", (7, 9, 5), ("upload", ("random", 11, 0.9, 0.4)), dict(tau_f=0.8, tau_g=0.6, alpha0=1.7, alpha1=0.3)),
        ("droplet7_split", (7, 9, 5), ("droplet", 0.3), dict(tau_f=0.5, tau_g=0.8, alpha0=2.5, kappa=1.0)),
        ("column_ulp", (1, 1, 8), ("stripe", 0.5), dict(tau_f=ONE_ULP_ABOVE, tau_g=ONE_ULP_ABOVE)),
        ("column_tau", (1, 1, 8), ("stripe", 0.5), dict(tau_f=0.8, tau_g=0.8)),
        ("small_above", (3, 5, 4), ("droplet", 0.3), dict(tau_f=hi, tau_g=hi, alpha0=2.5, kappa=1.0)),
        ("small_below", (3, 5, 4), ("droplet", 0.3), dict(tau_f=lo, tau_g=0.5, alpha0=4.0, kappa=0.1)),
        ("small_random", (3, 5, 4), ("upload", ("random", 5, 0.9, 0.4)), dict(alpha0=1.5)),
        ("pair", (2, 1, 1), ("upload", ("random", 3, 0.9, 0.4)), dict(tau_f=0.8, tau_g=0.6, alpha0=1.5)),
        ("pair_half", (2, 1, 1), ("upload", ("random", 4, 0.5, 0.7)), dict(alpha0=4.0)),
        ("pair_stripe", (2, 1, 1), ("stripe", 0.5), dict(tau_f=1.0, tau_g=1.0)),
    ]
    return [dict(name=nm, n=n, init=init, par=par, steps=10, dump=STEPS) for nm, n, init, par in c]


def tiling_cases():
    return [
        dict(name="edge65", n=(65, 9, 3), init=("droplet", 0.47), par=dict(), steps=10, dump=STEPS),
        dict(name="edge65_tau", n=(65, 9, 3), init=("stripe", 0.5), par=dict(tau_f=0.8, tau_g=0.6, alpha0=2.5), steps=10, dump=STEPS),
        dict(name="handover64", n=(64, 8, 9), init=("droplet", 0.45), par=dict(), steps=10, dump=(0, 1, 10), keep={10: ("hbar", "h")}),
        dict(name="handover64_tau", n=(64, 8, 9), init=("droplet", 0.45), par=dict(tau_f=0.8, tau_g=0.6, alpha0=2.5), steps=10,
             dump=(0, 1, 10), keep={10: ("hbar", "h")}),
    ]


def noise_cases():
    """table "numpy": seeded standard normals, the noise of every step is stored for injection.  table "project": the
    project's own stream in the reference's call order; stored are the densities and the reference's noise field."""
    inj = [
        ("mixture_inj", (3, 4, 5), ("mixture",), dict(tau_f=1.0, tau_g=1.0, alpha0=0.0, kBT=1e-5), 10, STEPS),
        ("droplet_inj", (5, 6, 4), ("droplet", 0.3), dict(tau_f=0.8, tau_g=0.6, alpha0=2.0, kBT=1e-5), 3, (0, 1, 3)),
        ("stripe_inj", (2, 3, 5), ("stripe", 0.5), dict(kBT=1e-6), 10, STEPS),
        ("signed_inj", (4, 3, 5), ("upload", ("signed", 21)), dict(tau_f=0.7, tau_g=0.9, alpha0=1.0, kBT=1e-5), 3, (0, 1, 3)),
    ]
    gen = [
        ("mixture_gen", (6, 5, 7), ("mixture",), dict(tau_f=1.0, tau_g=1.0, alpha0=0.0, kBT=1e-5), 2, (0, 2)),
        ("droplet_gen", (6, 5, 7), ("droplet", 0.3), dict(tau_f=0.8, tau_g=0.6, alpha0=2.0, kBT=1e-5), 2, (0, 2)),
        ("droplet_gen_half", (6, 5, 7), ("droplet", 0.3), dict(kBT=1e-6), 0, (0,)),
        ("mixture_gen_half", (5, 4, 9), ("mixture",), dict(alpha0=0.0, kBT=1e-5), 0, (0,)),
        ("signed_gen", (4, 3, 5), ("upload", ("signed", 22)), dict(tau_f=0.8, tau_g=0.6, alpha0=1.0, kBT=1e-5), 0, (0,)),
    ]
    out = [dict(name=nm, n=n, init=i, par=p, steps=s, dump=d, table="numpy") for nm, n, i, p, s, d in inj]
    out += [dict(name=nm, n=n, init=i, par=p, steps=s, dump=d, table="project", seed=SEED) for nm, n, i, p, s, d in gen]
    return out


REFSTATE_N = (5, 4, 6)
REFSTATE_PAR = dict(tau_f=0.8, tau_g=0.6, kBT=1e-5)
REFSTATE_SHIFTS = {
    "zero": (0.0, 0.0, 0.0),
    "fraction": (0.9, -0.9, 0.5),            # truncates to zero on every axis
    "negative": (-2.6, -1.4, -3.3),
    "mixed": (2.6, -1.4, 3.3),
    "beyond_half": (3.7, 3.2, 4.2),          # trunc = (3, 3, 4) on 5 x 4 x 6
    "almost_box": (4.9, -3.9, 5.9),          # trunc = (4, -3, 5): the largest shift the single wrap keeps in range
}


# ---- running the reference -----------------------------------------------------------------------------------------

def stability(case):
    """alpha0 x (rho_hi + rho_lo) <= 6, the project's own bound; for an upload the largest rho + phi of the state."""
    alpha0 = case["par"].get("alpha0", 4.0)
    if case["init"][0] == "upload":
        f0, g0 = upload_state(case["n"], case["init"][1])
        total = float(np.abs(f0.sum(0) + g0.sum(0)).max())
    else:
        total = 1.0                                              # the reference's rho_hi + rho_lo
    return abs(alpha0) * total


def run_case(case):
    import reference_binding as rb
    n, steps = case["n"], case["steps"]
    ns = n[0] * n[1] * n[2]
    init, f0g0 = case["init"], None
    if init[0] == "upload":
        f0g0 = upload_state(n, init[1])
        init = ("file",) + f0g0
    normals = None
    if case.get("table") == "numpy":
        normals = np.random.default_rng(sum(map(ord, case["name"]))).standard_normal((steps + 1, ns, 33))
    elif case.get("table") == "project":
        normals = project_normals(n, steps, case["seed"])
    noisy = normals is not None
    rec = rb.run(n, case["par"], init, steps, range(steps + 1) if noisy else case["dump"], normals=normals)
    return rec, f0g0


def store(out, case, rec, f0g0):
    name, n = case["name"], case["n"]
    ns = n[0] * n[1] * n[2]
    assert stability(case) <= 6.0 + 1e-12, (name, stability(case))
    if f0g0 is not None:
        out[f"{name}/f0"], out[f"{name}/g0"] = f0g0
    keep = {int(k): v for k, v in case.get("keep", {}).items()}
    for s, r in rec.items():
        for nm, arr in r.items():
            assert np.isfinite(arr).all(), f"{name}: the reference alone gives NaN/Inf in {nm} at step {s}"
        if s in case["dump"]:
            for nm in ("f", "g", "hbar", "h"):
                key = f"{name}/{s}/{nm}"
                if nm in keep.get(s, ()):
                    out[key] = r[nm][:9]                              # what tests/tolerances.py reads: comps 0..8
                    out[key + "_digest"] = digest(r[nm])
                else:
                    out[key] = r[nm] if ns <= FULL_ARRAYS_UP_TO else digest(r[nm])
        if case.get("table") == "numpy":
            out[f"{name}/{s}/fn"], out[f"{name}/{s}/gn"] = r["fn"], r["gn"]
        elif case.get("table") == "project" and s in case["dump"]:
            out[f"{name}/{s}/fn"], out[f"{name}/{s}/gn"] = r["fn"], r["gn"]
            out[f"{name}/{s}/rho"], out[f"{name}/{s}/phi"] = r["hbar"][0], r["hbar"][1]


def describe(cases):
    import reference_binding as rb
    info = rb.build_info()
    return dict(compiler=info[0], flags=info[1], cases={c["name"]: {k: v for k, v in c.items() if k != "name"} for c in cases})


def write(name, out, meta):
    out = {k.replace("/", "__"): v for k, v in out.items()}
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(path(name), **out)
    print(f"{os.path.basename(path(name))}: {len(out)} entries, {os.path.getsize(path(name))} bytes")


def build_runs(name, cases):
    out = {}
    for case in cases:
        rec, f0g0 = run_case(case)
        store(out, case, rec, f0g0)
    write(name, out, describe(cases))


def build_units():
    import oracle_binding as ob
    import reference_binding as rb
    out = {}
    rng = np.random.default_rng(7)
    K = 64
    vec = rng.uniform(-0.5, 1.0, (K, 19))
    fields = rng.uniform(0.05, 2.0, (K, 2))
    u = rng.uniform(-0.3, 0.3, (K, 3))
    a = rng.uniform(-0.1, 0.1, (K, 3))
    vec[0] = 0.0; fields[1] = (0.0, 1.0); u[2] = 0.0; a[3] = 0.0           # exact zeros take their own paths
    meta = dict(describe([]), units={}, refstate=dict(n=REFSTATE_N, par=REFSTATE_PAR, shifts=REFSTATE_SHIFTS, seed=SEED))
    for tag, tau_f, shape in (("half", 0.5, (5, 4, 6)), ("tau", 0.8, (1, 3, 2)), ("line", ONE_ULP_ABOVE, (7, 1, 1))):
        field = rng.uniform(-1.0, 2.0, shape[::-1])
        res = rb.units(vec, fields, u, a, field, tau_f=tau_f)
        assert all(np.isfinite(v).all() for v in res.values())
        meta["units"][tag] = dict(tau_f=tau_f, n=shape)
        for nm, arr in dict(vec=vec, fields=fields, u=u, a=a, field=field, **res).items():
            out[f"unit/{tag}/{nm}"] = arr
    # reference-state noise: the USE_REF_STATE build's thermal_noise, the project's stream at noise index 0
    n = REFSTATE_N
    normals = project_normals(n, 0)
    for kind, signed in (("positive", False), ("signed", True)):
        ref = ref_fields(n, 3, signed)
        for nm, arr in zip(("rho_eq", "phi_eq", "rhot_eq"), ref):
            out[f"refstate/{kind}/{nm}"] = arr
        for tag, shift in REFSTATE_SHIFTS.items():
            assert all(abs(np.trunc(s)) < e for s, e in zip(shift, n))     # the reference wraps once only: stay inside one box length
            dummy = np.ones(n[::-1])                                       # hydrovsbar is not read by this build
            fn, gn = rb.thermal_noise(n, REFSTATE_PAR, dummy, dummy, normals, refstate=ref, shift=shift)
            assert np.isfinite(fn).all() and np.isfinite(gn).all()
            out[f"refstate/{kind}/{tag}/fn"], out[f"refstate/{kind}/{tag}/gn"] = fn, gn
    write("units", out, meta)


if __name__ == "__main__":
    import reference_binding as rb
    if not rb.available():
        sys.exit("oracle/_ref/ is not built: make -C oracle/ref_harness (needs the reference's headers)")
    build_runs("trajectories", trajectory_cases())
    build_runs("noise_injected", [c for c in noise_cases() if c["table"] == "numpy"])
    build_runs("noise_generated", [c for c in noise_cases() if c["table"] == "project"])
    build_runs("tiling", tiling_cases())
    build_units()
