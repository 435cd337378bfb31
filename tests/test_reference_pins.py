"""CPU: the oracle against the REFERENCE's own compiled code.

oracle/bflbm_oracle.c restates LBM_d3q19.H / LBM_binary.H by hand; the GPU suite proves the kernels equal to it.  Here
the restatement itself is compared with what the reference's headers compute when compiled unmodified against
oracle/ref_harness/amrex_lite.H (g++ -std=c++17 -O2 -ffp-contract=off, no -march):

  from fixtures (tests/golden/reference_*.npz, always run)
    * every recorded trajectory: init and all recorded steps of f, g, hydrovsbar (15) and hydrovs (22) equal as numbers
      (x + 0.0, NaN-aware); cases with kBT > 0 are driven with the reference's recorded noise of every step;
    * the six site functions on seeded random inputs, bit for bit;
    * the oracle's GENERATED noise on the reference's own state against the reference's field from the same normals,
      plain and USE_REF_STATE branch, in ulp (bound derived in reference_fixtures.NOISE_ULP_BOUND);
  live (needs oracle/_ref/, which build() makes where the reference's headers exist; skipped only without it)
    * 40 seeded draws of lattice, init, parameters and step count against the binary, the same equality;
    * SURVEY 8c's three numbers from the binary's own printout.

Measured maxima of the noise comparison (this file, fixtures as committed): plain branch 2 ulp, USE_REF_STATE branch 2 ulp.
"""
import numpy as np
import pytest

import reference_binding as rb
import reference_fixtures as rf

LIVE = pytest.mark.skipif(not rb.available(), reason="oracle/_ref/ is not built (the reference's headers are not on this machine)")


def _oracle(ob, case, z, name, **extra):
    par = dict(case["par"], **extra)
    o = ob.OracleLattice(*case["n"], params=ob.default_params(**par))
    state = rf.initial_state(z, name, case)
    if state is not None:
        o.init_from(*state)
    else:
        getattr(o, "init_" + case["init"][0])(*case["init"][1:])
    return o


def _record(o):
    return dict(f=o.f, g=o.g, hbar=o.hbar, h=o.h)


def _quiet_cases():
    return [(fx, nm) for fx in ("trajectories", "tiling") for nm in rf.cases(fx)]


def test_fixtures_describe_themselves_and_are_finite():
    for fx in rf.FILES:
        meta, z = rf.fixture(fx)
        assert "g++" in meta["compiler"] and "-ffp-contract=off" in meta["flags"] and "-march" not in meta["flags"]
        for k, v in z.items():
            assert v.dtype == np.uint8 or np.isfinite(v).all(), (fx, k)
        for nm, case in meta["cases"].items():
            assert {"n", "par", "init", "steps", "dump"} <= set(case), (fx, nm)


@pytest.mark.parametrize("fx,name", _quiet_cases())
def test_oracle_trajectory_equals_the_reference(ob, fx, name):
    meta, z = rf.fixture(fx)
    case = meta["cases"][name]
    assert case["par"].get("kBT", 0.0) == 0.0
    o = _oracle(ob, case, z, name)
    done = 0
    for s in case["dump"]:
        while done < s:
            o.timestep(); done += 1
        rf.assert_record(z, f"{name}/{s}", _record(o), f"{name} step {s}")


@pytest.mark.parametrize("name", list(rf.cases("noise_injected")))
def test_oracle_with_the_references_noise_equals_the_reference(ob, name):
    """The reference ran with kBT > 0 on a table of normals; its noise fields of every step drive the oracle."""
    meta, z = rf.fixture("noise_injected")
    case = meta["cases"][name]
    o = _oracle(ob, case, z, name)
    noise = lambda s: (z[f"{name}/{s}/fn"], z[f"{name}/{s}/gn"])
    assert np.abs(noise(0)[0]).max() > 0
    o.set_noise(*noise(0))
    rf.assert_record(z, f"{name}/0", _record(o), f"{name} step 0")
    for s in range(1, case["steps"] + 1):
        o.timestep_injected(*noise(s - 1), *noise(s))
        if s in case["dump"]:
            rf.assert_record(z, f"{name}/{s}", _record(o), f"{name} step {s}")


@pytest.mark.parametrize("tag", list(rf.fixture("units")[0]["units"]))
def test_site_functions_equal_the_reference_bit_for_bit(ob, tag):
    meta, z = rf.fixture("units")
    par = ob.default_params(tau_f=meta["units"][tag]["tau_f"])
    g = lambda nm: z[f"unit/{tag}/{nm}"]
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    vec, fields, u, a = g("vec"), g("fields"), g("u"), g("a")
    got = {
        "moments": np.array([ob.moments(v) for v in vec]),
        "populations": np.array([ob.populations(v) for v in vec]),
        "gradient": ob.gradient(g("field"), par),
        "grad_laplacian_2nd": ob.grad_laplacian_2nd(g("field"), par),
    }
    for idx in (0, 1):
        got[f"equilibrium_moments_{idx}"] = np.array([ob.equilibrium_moments(fields[k], idx, u[k], par) for k in range(len(vec))])
        got[f"phi_moments_{idx}"] = np.array([ob.phi_moments(fields[k], idx, u[k], a[k], par) for k in range(len(vec))])
    for nm, arr in got.items():
        assert np.array_equal(bits(arr), bits(g(nm))), f"{tag}: {nm} differs from the reference in {np.count_nonzero(bits(arr) != bits(g(nm)))} doubles"


def test_generated_noise_on_the_references_state(ob):
    """Plain branch (LBM_binary.H:109-111): the oracle's thermal_noise on the reference's rho, phi with the project's
    stream, against the reference's field from the same normals in its own call order.  Bound: NOISE_ULP_BOUND."""
    meta, z = rf.fixture("noise_generated")
    worst = 0.0
    for name, case in meta["cases"].items():
        par = ob.default_params(seed=case["seed"], **case["par"])
        for s in case["dump"]:
            fn, gn = ob.thermal_noise(case["n"], par, z[f"{name}/{s}/rho"], z[f"{name}/{s}/phi"], noise_index=s)
            worst = max(worst, rf.assert_noise(fn, gn, z[f"{name}/{s}/fn"], z[f"{name}/{s}/gn"], f"{name} step {s}"))
    print(f"[noise ulp] plain branch, all cases: max {worst:g} ulp")
    assert any((z[f"{nm}/0/rho"] < 0).any() and (z[f"{nm}/0/phi"] < 0).any() for nm in meta["cases"]), "no case reaches the abs()"


@pytest.mark.parametrize("kind", ["positive", "signed"])
def test_generated_noise_of_the_reference_state_branch(ob, kind):
    """USE_REF_STATE (:92-107): densities from the equilibrium fields at the site shifted by trunc(pos_com_relative),
    wrapped once.  Shifts: zero, a fraction (truncates to zero), negative, mixed signs, beyond half the box, and the
    largest the single wrap keeps in range; `signed` fields take the abs() of every amplitude."""
    meta, z = rf.fixture("units")
    info = meta["refstate"]
    par = ob.default_params(seed=info["seed"], **info["par"])
    ref = [z[f"refstate/{kind}/{nm}"] for nm in ("rho_eq", "phi_eq", "rhot_eq")]
    assert kind == "positive" or ((ref[0] < 0).any() and (ref[1] < 0).any())
    worst, fields = 0.0, {}
    for tag, shift in info["shifts"].items():
        fn, gn = ob.thermal_noise(info["n"], par, None, None, noise_index=0, ref=ref, rel=shift)
        want = z[f"refstate/{kind}/{tag}/fn"], z[f"refstate/{kind}/{tag}/gn"]
        worst = max(worst, rf.assert_noise(fn, gn, *want, f"USE_REF_STATE {kind} shift {tag}"))
        fields[tag] = want[0]
    print(f"[noise ulp] USE_REF_STATE branch, {kind}: max {worst:g} ulp")
    assert rf.same(fields["zero"], fields["fraction"])                       # static_cast<int> truncates toward zero
    assert not rf.same(fields["zero"], fields["negative"]) and not rf.same(fields["mixed"], fields["negative"])


# ---- live: the binary itself ---------------------------------------------------------------------------------------

def _draw(i):
    """Draw i: a non-cubic lattice with extents 1..24 (at most 2000 sites), an init, tau_f != tau_g, alpha0 inside the
    stability bound alpha0 x (rho + phi) <= 6 (the analytic inits have rho + phi = 1, the uploads at most 1.7), alpha1,
    kappa, kBT and a step count <= 12."""
    rng = np.random.default_rng(1000 + i)
    while True:
        n = tuple(int(v) for v in rng.integers(1, 25, 3))
        if len(set(n)) > 1 and n[0] * n[1] * n[2] <= 2000:
            break
    kind = ("stripe", "droplet", "mixture", "upload")[i % 4]
    tau_f = 0.5 if i % 5 == 0 else float(rng.uniform(0.5, 1.2))
    tau_g = float(rng.uniform(0.5, 1.2))
    assert tau_f != tau_g
    par = dict(tau_f=tau_f, tau_g=tau_g, alpha0=float(rng.uniform(0.0, 3.5 if kind == "upload" else 5.0)),
               alpha1=float(rng.uniform(-1.0, 1.0)), kappa=float(rng.uniform(0.1, 4.0)),
               kBT=float((0.0, 0.0, 1e-6, 1e-5)[int(rng.integers(0, 4))]))
    if kind == "upload":
        w = np.array([1 / 3] + [1 / 18] * 6 + [1 / 36] * 12)[:, None, None, None]
        shp = (19, n[2], n[1], n[0])
        init = ("file", w * (0.9 + 0.2 * rng.random(shp)), w * (0.4 + 0.2 * rng.random(shp)))
    elif kind == "mixture":
        init = ("mixture",)
    else:
        init = (kind, float(rng.uniform(0.2, 0.6)))
    return n, par, init, int(rng.integers(1, 13)), rng


@LIVE
@pytest.mark.parametrize("i", range(40))
def test_live_draw_equals_the_reference_binary(ob, i):
    n, par, init, steps, rng = _draw(i)
    noisy = par["kBT"] > 0
    normals = rng.standard_normal((steps + 1, n[0] * n[1] * n[2], 33)) if noisy else None
    ref = rb.run(n, par, init, steps, range(steps + 1), normals=normals)
    o = ob.OracleLattice(*n, params=ob.default_params(**par))
    if init[0] == "file":
        o.init_from(init[1], init[2])
    else:
        getattr(o, "init_" + init[0])(*init[1:])
    what = f"draw {i}: {n} {init[0]} {par} "
    if noisy:
        o.set_noise(ref[0]["fn"], ref[0]["gn"])
    for s in range(steps + 1):
        if s:
            if noisy:
                o.timestep_injected(ref[s - 1]["fn"], ref[s - 1]["gn"], ref[s]["fn"], ref[s]["gn"])
            else:
                o.timestep()
        for nm, arr in _record(o).items():
            assert rf.same(arr, ref[s][nm]), what + f"step {s}: {nm}: " + rf.mismatch(arr, ref[s][nm])


@LIVE
def test_live_binary_prints_the_survey_numbers():
    """8^3 stripe 0.5, header defaults, 10 steps."""
    _, text = rb.run((8, 8, 8), {}, ("stripe", 0.5), 10, [10], stdout=True)
    assert text.split() == ["mass", "511.99999999999886", "rho(0,0,4)", "1.0185845986909126", "ufz(0,0,2)", "0.048022250265876899"]


@LIVE
def test_live_fixtures_are_what_the_binary_writes_today():
    """The committed files against a fresh run of the generator's cases (one trajectory file's worth: 18 cases)."""
    meta, z = rf.fixture("trajectories")
    for name, case in meta["cases"].items():
        case = dict(case, name=name)
        rec, _ = rf.mgr.run_case(case)
        for s in case["dump"]:
            rf.assert_record(z, f"{name}/{s}", {k: rec[s][k] for k in ("f", "g", "hbar", "h")}, f"{name} step {s}")
