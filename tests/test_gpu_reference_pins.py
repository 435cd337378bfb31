"""GPU: the HIP kernels against the REFERENCE's own compiled code, not against the oracle.

Fixtures: tests/golden/reference_*.npz (LBM_d3q19.H / LBM_binary.H compiled unmodified against
oracle/ref_harness/amrex_lite.H; written by tests/golden/make_golden_reference.py).  Live: oracle/_ref/ref_main, when
the built binary came along with the tree, as a CPU subprocess.  The reference's directory itself is never read.

  * exact schedules (two_pass, fused) and 3-replica batches: the fixture's step-0 state (uploaded where the fixture
    stores one, else the same analytic init, whose result must equal the reference's step 0), the reference's recorded
    noise injected where present; values or digests equal at every recorded step;
  * hand-over schedule on 64 x 8 x 9: step 0 and 1 equal, step 10 under tolerances.check(..., 1e-12) against the
    reference's hydrovsbar and hydrovs;
  * thermal_noise() of a fresh context (project's stream, seed, noise index 0) against the reference's field from the
    same normals, default schedule and two_pass, tau = 1/2 and tau != 1/2, mixture, droplet and a state with densities
    of both signs; the USE_REF_STATE branch for six shifts.  Bound: reference_fixtures.NOISE_ULP_BOUND.
"""
import numpy as np
import pytest

import reference_binding as rb
import reference_fixtures as rf
import tolerances

pytestmark = pytest.mark.gpu
EXACT = ["two_pass", "fused"]
LIVE = pytest.mark.skipif(not rb.available(), reason="oracle/_ref/ did not come with the tree")


def _init(lat, case, state):
    if state is not None:
        lat.LBM_init(np.ascontiguousarray(state[0]), np.ascontiguousarray(state[1]))
    elif case["init"][0] == "mixture":
        lat.LBM_init_mixture()
    else:
        getattr(lat, "LBM_init_" + case["init"][0])(case["init"][1])


def _start(pkg, case, z, name, schedule, **extra):
    lbm = pkg.BinaryLBM(*case["n"], params=pkg.default_params(**dict(case["par"], **extra)), schedule=schedule)
    _init(lbm, case, rf.initial_state(z, name, case))
    return lbm


def _record(lat):
    f, g = lat.populations()
    hb9 = lat.LBM_hydrovars_density()
    hbar = np.zeros((15,) + hb9.shape[1:])           # the driver allocates 15 components; the path writes 0..8
    hbar[:9] = hb9
    return dict(f=f, g=g, hbar=hbar, h=lat.LBM_hydrovars())


def _advance(lat, upto):
    if upto > lat.steps_done:
        lat.LBM_timestep(upto - lat.steps_done)


def _quiet(fixtures, only=None):
    return [(fx, nm) for fx in fixtures for nm in rf.cases(fx) if only is None or nm.startswith(only)]


@pytest.mark.parametrize("schedule", EXACT)
@pytest.mark.parametrize("fx,name", _quiet(("trajectories", "tiling")))
def test_exact_schedules_equal_the_reference(pkg, fx, name, schedule):
    meta, z = rf.fixture(fx)
    case = meta["cases"][name]
    with _start(pkg, case, z, name, schedule) as lbm:
        assert lbm.resolved_schedule() == schedule
        for s in case["dump"]:
            _advance(lbm, s)
            rf.assert_record(z, f"{name}/{s}", _record(lbm), f"{name} {schedule} step {s}")


@pytest.mark.parametrize("schedule", EXACT)
@pytest.mark.parametrize("name", list(rf.cases("noise_injected")))
def test_exact_schedules_with_the_references_noise(pkg, name, schedule):
    """kBT > 0: the noise field the reference drew before each step is injected; hydrovs (which reads the noise of modes
    1..3) is compared with the same field injected."""
    meta, z = rf.fixture("noise_injected")
    case = meta["cases"][name]
    with _start(pkg, case, z, name, schedule) as lbm:
        for s in range(case["steps"] + 1):
            lbm.inject_noise(np.ascontiguousarray(z[f"{name}/{s}/fn"]), np.ascontiguousarray(z[f"{name}/{s}/gn"]))
            if s in case["dump"]:
                rf.assert_record(z, f"{name}/{s}", _record(lbm), f"{name} {schedule} step {s}")
            if s < case["steps"]:
                assert lbm.resolved_schedule() == schedule
                lbm.LBM_timestep(1)


def _batches():
    by_shape = {}
    for name, case in rf.cases("trajectories").items():
        by_shape.setdefault(tuple(case["n"]), []).append(name)
    return [tuple(names[-3:]) for names in by_shape.values() if len(names) >= 3]


@pytest.mark.parametrize("schedule", EXACT)
@pytest.mark.parametrize("names", _batches(), ids="+".join)
def test_three_replica_batch_equals_the_reference(pkg, names, schedule):
    meta, z = rf.fixture("trajectories")
    cases = [meta["cases"][nm] for nm in names]
    with pkg.BatchLBM(cases[0]["n"], params=[c["par"] for c in cases], schedule=schedule) as b:
        assert b.resolved_schedule() == schedule and len(b) == 3
        for rep, nm, case in zip(b.replicas, names, cases):
            _init(rep, case, rf.initial_state(z, nm, case))
        done = 0
        for s in cases[0]["dump"]:
            if s > done:
                b.LBM_timestep(s - done); done = s
            for rep, nm in zip(b.replicas, names):
                rf.assert_record(z, f"{nm}/{s}", _record(rep), f"batch {schedule} replica {nm} step {s}")


@pytest.mark.parametrize("name", [nm for nm in rf.cases("tiling") if nm.startswith("handover")])
def test_handover_schedule_against_the_reference(pkg, name):
    """The hand-over schedule's contract: the first step after an init equals the reference, later steps stay within
    the 1e-12 metric of tests/tolerances.py -- here against the reference's own arrays."""
    meta, z = rf.fixture("tiling")
    case = meta["cases"][name]
    with _start(pkg, case, z, name, "handover") as lbm:
        assert lbm.resolved_schedule() == "handover"
        for s in (0, 1):
            _advance(lbm, s)
            rf.assert_record(z, f"{name}/{s}", _record(lbm), f"{name} hand-over step {s}")
        _advance(lbm, 10)
        assert lbm.resolved_schedule() == "handover"
        rec = _record(lbm)
    for nm in ("hbar", "h"):
        e = tolerances.errors(rec[nm], z[f"{name}/10/{nm}"])
        print(f"[hand-over against the reference] {name} step 10 {nm}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        tolerances.check(rec[nm], z[f"{name}/10/{nm}"], f"{name} hand-over step 10 {nm}", 1e-12)


@pytest.mark.parametrize("schedule", [None, "two_pass"], ids=["default", "two_pass"])
@pytest.mark.parametrize("name", list(rf.cases("noise_generated")))
def test_generated_noise_against_the_references_field(pkg, name, schedule):
    meta, z = rf.fixture("noise_generated")
    case = meta["cases"][name]
    with _start(pkg, case, z, name, schedule, seed=case["seed"]) as lbm:
        hb = lbm.LBM_hydrovars_density()
        assert rf.same(hb[0], z[f"{name}/0/rho"]) and rf.same(hb[1], z[f"{name}/0/phi"]), f"{name}: densities differ from the reference"
        fn, gn = lbm.thermal_noise()
    rf.assert_noise(fn, gn, z[f"{name}/0/fn"], z[f"{name}/0/gn"], f"GPU {name} {schedule or 'default'}")


@pytest.mark.parametrize("kind", ["positive", "signed"])
def test_reference_state_noise_against_the_references_field(pkg, ob, kind):
    """USE_REF_STATE: the kernel's lookup at the site shifted by trunc(COM - com_ref) and its amplitudes from the
    equilibrium fields.  com_ref is placed so that COM - com_ref is the fixture's shift (the centre of mass itself is
    the project's; the reference binary was given the shift)."""
    meta, z = rf.fixture("units")
    info = meta["refstate"]
    nx, ny, nz = info["n"]
    ref = [z[f"refstate/{kind}/{nm}"] for nm in ("rho_eq", "phi_eq", "rhot_eq")]
    tmp = ob.OracleLattice(nx, ny, nz, ob.default_params(**info["par"]))
    tmp.init_droplet(0.3)
    for tag, shift in info["shifts"].items():
        if tag == "fraction":
            continue                                  # 0.9 off an integer is fine, but zero covers the same lookup
        with pkg.BinaryLBM(nx, ny, nz, params=pkg.default_params(seed=info["seed"], **info["par"])) as lbm:
            lbm.set_ref_state(*ref, com_ref=tmp.com() - np.asarray(shift))
            lbm.LBM_init(tmp.f, tmp.g)
            assert lbm.ref_state_active
            fn, gn = lbm.thermal_noise()
        rf.assert_noise(fn, gn, z[f"refstate/{kind}/{tag}/fn"], z[f"refstate/{kind}/{tag}/gn"], f"GPU USE_REF_STATE {kind} shift {tag}")


# ---- live: shapes too big to commit --------------------------------------------------------------------------------

@LIVE
@pytest.mark.parametrize("tau", [(0.5, 0.5), (0.8, 0.6)], ids=["half", "0.8-0.6"])
@pytest.mark.parametrize("n,init", [((70, 11, 9), ("droplet", 0.45)), ((130, 17, 5), ("stripe", 0.5)), ((8, 70, 6), ("droplet", 0.6))],
                         ids=["70x11x9", "130x17x5", "8x70x6"])
def test_live_reference_binary_against_the_exact_schedules(pkg, n, init, tau):
    par = dict(tau_f=tau[0], tau_g=tau[1], alpha0=2.5)
    ref = rb.run(n, par, init, 5, (0, 1, 5))
    for schedule in EXACT:
        with pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule=schedule) as lbm:
            getattr(lbm, "LBM_init_" + init[0])(init[1])
            for s in (0, 1, 5):
                _advance(lbm, s)
                for nm, arr in _record(lbm).items():
                    assert rf.same(arr, ref[s][nm]), f"{n} {schedule} tau {tau} step {s}: {nm}: " + rf.mismatch(arr, ref[s][nm])


@LIVE
def test_live_generated_noise_where_the_default_schedule_generates_it_itself(pkg):
    """64 x 8 x 16 with kBT > 0: full hand-over tiles, so `auto` may run the kernel with the generator inside; the noise
    observable of the fresh context against the reference binary fed the project's stream."""
    n, par = (64, 8, 16), dict(tau_f=0.8, tau_g=0.6, alpha0=2.0, kBT=1e-5)
    normals = rf.mgr.project_normals(n, 0)
    ref = rb.run(n, par, ("droplet", 0.4), 0, (0,), normals=normals)[0]
    with pkg.BinaryLBM(*n, params=pkg.default_params(seed=rf.mgr.SEED, **par)) as lbm:
        lbm.LBM_init_droplet(0.4)
        print("default schedule on 64 x 8 x 16 with noise:", lbm.resolved_schedule())
        fn, gn = lbm.thermal_noise()
    rf.assert_noise(fn, gn, ref["fn"], ref["gn"], "GPU 64x8x16 default schedule")
