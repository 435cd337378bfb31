"""GPU: replica batches under the launch plans of large batches, against the CPU oracle, bit for bit.

The other batch tests run at most 5 replicas (16 in one interface test), which the chunk planner always cuts into chunks of
2 planes on the narrow tiles (tests/test_batch_plans.py pins that).  Here many replicas of tiny lattices put every tile
family of k_fused_batch / k_fused_batch_unit -- 8x64, 16x32, 32x16, 64x8 quiet and the 32x8 noise tile, each with four tile
columns per replica, ragged in x and y -- under
  long:    one chunk of 8 planes (10 march positions: the four-slot density ring wraps twice), 172 workgroups, the
           launched grid padded by 4 workgroups that must leave;
  ragged:  chunks of 4, 4, 3 planes, 396 workgroups = 2 rounds, padded by 4, XCD part boundaries inside replicas;
  tail:    chunks of 3, 3, 1;
  full:    one chunk of 14 planes, exactly 256 workgroups, no padding (32x16 and the noise tile).
Every case first asserts, through the library's own planner (fused_plan_query), that the device has the 256 compute units
the table was chosen for and that the case has its regime; then every replica must hold the doubles of its own
OracleLattice (same parameters, seed, init).  There is no tolerance: the exact schedules' contract is bit identity.
Further: B = 130 through the two-pass kernels (replica in gridDim.z), the column order of fused_col with a narrower last
strip (ntx = 5, 6, 7), and a replica whose noise index crosses 2^32 inside a batch."""
import numpy as np
import pytest

import batch_plan_cases as bp

pytestmark = pytest.mark.gpu

STEPS = 3

# replicas differ in alpha0, kappa, rho_hi and tau (tau_f != tau_g in some): the generic kernels
GENERIC = [dict(alpha0=1.5, kappa=0.1, rho_hi=3.0),
           dict(alpha0=1.7, kappa=1.0, rho_hi=3.0, tau_f=0.7, tau_g=0.7),
           dict(alpha0=2.0, kappa=3.0, rho_hi=2.0, rho_lo=0.1),
           dict(alpha0=1.0, kappa=4.0, rho_hi=1.0, tau_f=0.6, tau_g=0.8),
           dict(alpha0=1.2, kappa=2.0, rho_hi=1.5, tau_f=0.55, tau_g=0.55)]
# every replica at the default tau = 1/2 (rho_lo = 0, the default, in some): the unit-rate kernels
UNIT = [dict(alpha0=1.5, kappa=0.1, rho_hi=3.0),
        dict(alpha0=2.0, kappa=3.0, rho_hi=2.0, rho_lo=0.1),
        dict(alpha0=1.0, kappa=4.0, rho_hi=1.0),
        dict(alpha0=1.2, kappa=2.0, rho_hi=1.5, rho_lo=0.05),
        dict(alpha0=1.7, kappa=1.0, rho_hi=3.0)]
KBT = [1e-5, 3e-5, 5e-6]
# six inits against five parameter sets: the pairing shifts from replica to replica
INITS = [("droplet", 0.2), ("stripe", 0.5), ("droplet", 0.3), ("mixture", None), ("perturbed", None), ("droplet", 0.4)]


@pytest.fixture()
def threads(ob):
    ob.lib().orc_set_threads(16)
    yield
    ob.lib().orc_set_threads(1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _replica_params(variant, nrep):
    """One parameter dict per replica, each with its own seed."""
    base = UNIT if variant == "unit" else GENERIC
    out = []
    for r in range(nrep):
        p = dict(base[r % len(base)], seed=1000 + 7 * r)
        if variant == "noise":
            p["kBT"] = KBT[r % len(KBT)]
        out.append(p)
    return out


def _oracles(ob, n, params, first_init=0):
    """One initialised OracleLattice per replica and the uploads of the 'perturbed' ones (replica -> (f0, g0))."""
    refs, uploads = [], {}
    for r, p in enumerate(params):
        ref = ob.OracleLattice(*n, params=ob.default_params(**p))
        kind, arg = INITS[(r + first_init) % len(INITS)]
        if kind == "perturbed":                                          # test_gpu_parity.py::test_degenerate_and_tile_edge_sizes
            rng = np.random.default_rng(50000 + r)
            ref.init_mixture()
            f0 = ref.f * (1.0 + 0.05 * rng.standard_normal(ref.f.shape))
            g0 = ref.g * (1.0 + 0.05 * rng.standard_normal(ref.g.shape))
            ref.init_from(f0, g0)
            uploads[r] = (f0.copy(), g0.copy())
        elif kind == "mixture":
            ref.init_mixture()
        else:
            getattr(ref, "init_" + kind)(arg)
        refs.append(ref)
    return refs, uploads


def _init_like(lat, r, uploads, first_init=0):
    kind, arg = INITS[(r + first_init) % len(INITS)]
    if kind == "perturbed":
        lat.LBM_init(*uploads[r])
    elif kind == "mixture":
        lat.LBM_init_mixture()
    else:
        getattr(lat, "LBM_init_" + kind)(arg)


def _report(name, got, want, bitwise):
    """Stacked arrays (B, components, nz, ny, nx): one line per replica that differs -- which component, how many doubles,
    which z-planes (a chunk seam shows in the planes, an error of the replica fold in the replicas)."""
    assert got.shape == want.shape, f"{name}: shape {got.shape}, expected {want.shape}"
    bad = (_bits(got) != _bits(want)) if bitwise else (got != want)
    lines = []
    for r in np.flatnonzero(bad.any(axis=(1, 2, 3, 4))):
        lines.append(f"replica {r}: {name}: {np.count_nonzero(bad[r])} of {bad[r].size} doubles differ, components "
                     f"{np.flatnonzero(bad[r].any(axis=(1, 2, 3))).tolist()}, z-planes {np.flatnonzero(bad[r].any(axis=(0, 2, 3))).tolist()}")
    return lines


def _compare(b, refs, what, noise):
    f, g = b.populations()
    want_f, want_g = np.stack([ref.f for ref in refs]), np.stack([ref.g for ref in refs])
    assert np.isfinite(want_f).all() and np.isfinite(want_g).all(), what + ": the oracle's run is not finite"
    lines = _report("f", f, want_f, True) + _report("g", g, want_g, True)
    lines += _report("hydrovs", b.LBM_hydrovars(), np.stack([ref.h for ref in refs]), False)
    lines += _report("hydrovsbar", b.LBM_hydrovars_density(), np.stack([ref.hbar[:9] for ref in refs]), False)
    if noise:
        fn, gn = (np.stack(a) for a in zip(*[rep.thermal_noise() for rep in b.replicas]))
        lines += _report("fnoise", fn, np.stack([ref.fn for ref in refs]), True)
        lines += _report("gnoise", gn, np.stack([ref.gn for ref in refs]), True)
    assert not lines, what + f": {len(lines)} differences\n" + "\n".join(lines[:40])
    assert np.array_equal(f, want_f) and np.array_equal(g, want_g), what                 # by value as well as by bits


def _run_batch(pkg, ob, n, params, schedule, steps, what, check_plan=None, first_init=0, before_step=None, expect_steps=None):
    noise = any(p.get("kBT", 0.0) != 0.0 for p in params)
    refs, uploads = _oracles(ob, n, params, first_init)
    with pkg.BatchLBM(n, params=params, schedule=schedule) as b:
        assert b.resolved_schedule() == schedule
        if check_plan is not None:
            plan = pkg.fused_plan_query(n, replicas=len(params), noise=noise, compute_units=0)
            assert plan["compute_units"] == bp.CUS, \
                f"the device reports {plan['compute_units']} compute units; the case table of batch_plan_cases.py was chosen for {bp.CUS}"
            check_plan(plan)
        for r, rep in enumerate(b.replicas):
            _init_like(rep, r, uploads, first_init)
        if before_step is not None:
            before_step(b, refs)
            _compare(b, refs, what + ", before the steps", noise)
        b.LBM_timestep(steps)                                             # one call: the records are written once
        for ref in refs:
            for _ in range(steps):
                ref.timestep()
        assert [rep.steps_done for rep in b.replicas] == [ref.steps for ref in refs] == (expect_steps or [steps] * len(refs))
        _compare(b, refs, what, noise)


def _variants(family):
    return ["noise"] if bp.FAMILIES[family]["noise"] else ["generic", "unit"]


@pytest.mark.parametrize("family,regime,variant", [(f, r, v) for f, r in bp.CASES for v in _variants(f)])
def test_every_tile_family_under_every_plan_regime(pkg, ob, threads, family, regime, variant):
    n, nrep, noise = bp.case_shape(family, regime)
    assert noise == (variant == "noise")
    _run_batch(pkg, ob, n, _replica_params(variant, nrep), "fused", STEPS, f"{family} {regime} {variant} {n} x {nrep}",
               check_plan=lambda plan: bp.check_case(plan, family, regime))


@pytest.mark.parametrize("variant", ["generic", "noise"])
def test_many_replicas_through_the_two_pass_kernels(pkg, ob, threads, variant):
    """B = 130 as gridDim.z of k_density_batch / k_collide_batch, and the stacked getters at that B."""
    n, nrep = (12, 10, 9), 130
    _run_batch(pkg, ob, n, _replica_params(variant, nrep), "two_pass", STEPS, f"two_pass {variant} {n} x {nrep}")


@pytest.mark.parametrize("tau", [(0.5, 0.5), (0.8, 0.6)])
@pytest.mark.parametrize("nrep", [1, 3])
@pytest.mark.parametrize("n,ntx", bp.STRIP_SHAPES)
def test_column_order_with_a_narrower_last_strip(pkg, ob, threads, n, ntx, nrep, tau):
    """fused_col with ntx = 5, 6, 7 at strips of 4 tiles: the last strip is 1, 2, 3 tiles wide.  A lone lattice and a
    3-replica batch, the unit-rate and the generic kernel, 4 steps."""
    par = dict(alpha0=1.5, kappa=1.0, rho_hi=2.0, tau_f=tau[0], tau_g=tau[1])
    what = f"{n} x {nrep} tau={tau}"
    if nrep > 1:
        params = [dict(par, alpha0=1.5 + 0.1 * r) for r in range(nrep)]
        _run_batch(pkg, ob, n, params, "fused", 4, what, check_plan=lambda plan: bp.check_strips(plan, n, ntx), first_init=4)
        return
    refs, uploads = _oracles(ob, n, [par], first_init=4)                  # the perturbed upload: no two tiles alike
    with pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule="fused") as lbm:
        assert lbm.resolved_schedule() == "fused"
        plan = pkg.fused_plan_query(n, replicas=1, noise=False, compute_units=0)
        bp.check_strips(plan, n, ntx)
        _init_like(lbm, 0, uploads, first_init=4)
        lbm.LBM_timestep(4)
        for _ in range(4):
            refs[0].timestep()
        f, g = lbm.populations()
        lines = _report("f", f[None], refs[0].f[None], True) + _report("g", g[None], refs[0].g[None], True)
        lines += _report("hydrovs", lbm.LBM_hydrovars()[None], refs[0].h[None], False)
        lines += _report("hydrovsbar", lbm.LBM_hydrovars_density()[None], refs[0].hbar[None, :9], False)
        assert not lines, what + "\n" + "\n".join(lines)
        assert np.array_equal(f, refs[0].f) and np.array_equal(g, refs[0].g), what


def test_noise_index_of_one_replica_crosses_2_to_the_32(pkg, ob, threads):
    """The batch kernels compute idx0 + (uint32_t)k: replica 1 starts two steps below 2^32 and takes 4 steps."""
    n, start = (6, 5, 7), 2 ** 32 - 2
    params = _replica_params("noise", 3)

    def shift(b, refs):
        b.replicas[1].set_steps_done(start)
        refs[1].steps = start
        refs[1].refresh()                                                 # the binding passes c_uint32(steps): the same wrap

    _run_batch(pkg, ob, n, params, "fused", 4, "across 2^32", before_step=shift, expect_steps=[4, 2 ** 32 + 2, 4])
