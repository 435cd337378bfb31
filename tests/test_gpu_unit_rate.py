"""GPU: the unit-rate quiet kernels (k_fused_unit, k_fused_ho_unit and the batch forms; csrc/bflbm_site.h,
d_relax_with<false, true>) against the CPU oracle, and the dispatch between them and the generic kernels.

A quiet launch takes the unit-rate kernels exactly when the derived rates inv_tau_f_bar and inv_tau_g_bar are both 1.0
(tau = 1/2, the header default).  They must store the generic kernels' bits, zeros with their SIGN included: the exact
schedules are compared with the oracle by value (np.array_equal) and by bit pattern on stripes, droplets in vacuum
(rho_lo = 0) and lattices that do not divide into the kernels' tiles.  Next to tau = 1/2: the double one ulp above it, whose
tau_bar still rounds to 1.0 -- the unit-rate kernels run on parameters derived from a tau that is NOT 1/2 --; the
nearest doubles on both sides whose rate is not 1.0 (one ulp below, two above) and tau = 1, which run the generic kernels;
all held to the same comparison.  Switching tau between steps switches kernels, which must leave no stale state (compared
with a fresh context).  The two-pass schedule of a lone lattice has no unit-rate kernel (csrc/bflbm_kernels.h); its cases
pin that the dispatch leaves it alone."""
import numpy as np
import pytest

from test_unit_rate_premise import nearest_tau_with_another_rate, unit_rate

pytestmark = pytest.mark.gpu

EXACT = ["two_pass", "fused"]
STEPS = 10
# lattices: a cube; ragged in x and y for the 64 x 8 tiles of schedule 1 and the 256-site blocks of schedule 0; the narrow
# lattices that run the 32 x 16, 16 x 32 and 8 x 64 tiles
CASES = [
    ((16, 16, 16), ("stripe", 0.5), {}),
    ((16, 16, 16), ("droplet", 0.3), dict(rho_lo=0.0)),
    ((70, 11, 9), ("stripe", 0.5), {}),
    ((70, 11, 9), ("droplet", 0.3), dict(rho_lo=0.0)),
    ((130, 17, 5), ("droplet", 0.2), dict(rho_lo=0.0)),
    ((24, 20, 8), ("droplet", 0.3), dict(rho_lo=0.0)),
    ((12, 36, 6), ("stripe", 0.5), {}),
    ((8, 70, 6), ("droplet", 0.4), dict(rho_lo=0.0)),
]
# the flat box whose droplet is centred outside it (LBM_init_droplet: z = nx/2) holds populations that are exactly zero, at
# init and after the steps: the case that makes the comparison of sign bits say something; asserted where it is run
VACUUM = ((130, 17, 5), "droplet")
ONE_ULP_ABOVE = float(np.nextafter(0.5, 1.0))
TAUS = [0.5, ONE_ULP_ABOVE, nearest_tau_with_another_rate(0.0), nearest_tau_with_another_rate(1.0), 1.0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what):
    assert np.array_equal(a, b), f"{what}: {np.count_nonzero(a != b)} of {a.size} doubles differ, max abs {np.nanmax(np.abs(a - b)):.3e}"
    sa, sb = np.signbit(a), np.signbit(b)
    assert np.array_equal(sa, sb), f"{what}: {np.count_nonzero(sa != sb)} sign bits differ (zeros of the other sign)"
    assert np.array_equal(_bits(a), _bits(b)), what


def _pair(pkg, ob, dims, init, schedule, par):
    lbm = pkg.BinaryLBM(*dims, params=pkg.default_params(**par), schedule=schedule)
    ref = ob.OracleLattice(*dims, params=ob.default_params(**par))
    getattr(lbm, "LBM_init_" + init[0])(*init[1:])
    getattr(ref, "init_" + init[0])(*init[1:])
    return lbm, ref


def _compare(lbm, ref, what):
    f, g = lbm.populations()
    _same_bits(f, ref.f, what + " f")
    _same_bits(g, ref.g, what + " g")
    # the observables come from k_observe, which this comparison does not pin to the oracle's signed zeros (its +-0.0 in
    # the velocity and acceleration fields differ from the oracle's with the generic step kernels too): values only
    assert np.array_equal(lbm.LBM_hydrovars(), ref.h), what + " hydrovs"


def test_the_taus_of_this_file_are_on_both_sides_of_the_dispatch():
    assert [bool(unit_rate(t) == 1.0) for t in TAUS] == [True, True, False, False, False]
    assert ONE_ULP_ABOVE != 0.5


@pytest.mark.parametrize("schedule", EXACT)
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("dims,init,par", CASES)
def test_exact_schedules_equal_the_oracle_sign_bits_included(pkg, ob, dims, init, par, tau, schedule):
    lbm, ref = _pair(pkg, ob, dims, init, schedule, dict(par, tau_f=tau, tau_g=tau))
    assert lbm.resolved_schedule() == schedule
    for s in range(STEPS):
        lbm.LBM_timestep(1)
        ref.timestep()
        if s in (0, STEPS - 1):
            _compare(lbm, ref, f"{dims} {init[0]} tau={tau!r} {schedule} step {s + 1}")
            if (dims, init[0]) == VACUUM:
                assert np.count_nonzero(ref.f == 0) > 1000, "the vacuum case holds no zeros"        # fluid f is the droplet's
    lbm.close()


@pytest.mark.parametrize("schedule", EXACT)
def test_only_one_unit_rate_runs_the_generic_kernel(pkg, ob, schedule):
    """tau_f = 1/2 with tau_g = 1 (and the reverse): one rate is 1.0, the other is not, so the generic kernel runs."""
    for tf, tg in ((0.5, 1.0), (1.0, 0.5)):
        lbm, ref = _pair(pkg, ob, (70, 11, 9), ("droplet", 0.3), schedule, dict(rho_lo=0.0, tau_f=tf, tau_g=tg))
        lbm.LBM_timestep(STEPS)
        for _ in range(STEPS):
            ref.timestep()
        _compare(lbm, ref, f"tau_f={tf} tau_g={tg} {schedule}")
        lbm.close()


@pytest.mark.parametrize("schedule", EXACT + ["handover"])
def test_switching_tau_between_steps_switches_kernels_without_stale_state(pkg, ob, schedule):
    """tau = 1 -> 1/2 -> 1 by bflbm_set_params between steps; after every leg the context equals a FRESH context that was
    handed the same populations and parameters (and, on the exact schedules, the oracle)."""
    dims = (128, 16, 16) if schedule == "handover" else (70, 11, 9)
    par = dict(rho_lo=0.0, alpha0=2.0)
    lbm, ref = _pair(pkg, ob, dims, ("droplet", 0.3), schedule, dict(par, tau_f=1.0, tau_g=1.0))
    assert lbm.resolved_schedule() == schedule
    for leg, tau in enumerate((1.0, 0.5, 1.0, 0.5)):
        if leg:
            lbm.set_params(tau_f=tau, tau_g=tau)
            ref.p.tau_f = ref.p.tau_g = tau
            ref.refresh()
        f0, g0 = lbm.populations()
        fresh = pkg.BinaryLBM(*dims, params=pkg.default_params(**dict(par, tau_f=tau, tau_g=tau)), schedule=schedule)
        fresh.LBM_init(f0, g0)
        lbm.LBM_timestep(4)
        fresh.LBM_timestep(4)
        for _ in range(4):
            ref.timestep()
        f, g = lbm.populations()
        ff, gf = fresh.populations()
        if schedule == "handover":
            # the fresh context pulls every ring on its first step, the running one reads frames: equal to the schedule's
            # tolerance (the first leg starts from an init on both sides and is bit-equal)
            assert np.allclose(f, ff, rtol=0, atol=1e-13) and np.allclose(g, gf, rtol=0, atol=1e-13), (leg, tau)
            assert np.allclose(f, ref.f, rtol=0, atol=1e-13) and np.allclose(g, ref.g, rtol=0, atol=1e-13), (leg, tau)
        else:
            _same_bits(f, ff, f"leg {leg} tau={tau} {schedule} f against a fresh context")
            _same_bits(g, gf, f"leg {leg} tau={tau} {schedule} g against a fresh context")
            _compare(lbm, ref, f"leg {leg} tau={tau} {schedule}")
        fresh.close()
    lbm.close()


@pytest.mark.parametrize("dims", [(128, 16, 16), (136, 18, 16)])       # full 64 x 4 tiles; a narrower last column and a lower last row
@pytest.mark.parametrize("tau", [0.5, 1.0])
def test_handover_first_step_is_the_exact_schedule_bit_for_bit(pkg, ob, dims, tau):
    """Schedule 3 pulls every ring on the first step after an init: the oracle's doubles, from k_fused_ho_unit at tau = 1/2
    and from k_fused_ho at tau = 1; later steps stay within the schedule's population tolerance (1e-13)."""
    par = dict(rho_lo=0.0, alpha0=2.0, tau_f=tau, tau_g=tau)
    lbm, ref = _pair(pkg, ob, dims, ("droplet", 0.3), "handover", par)
    assert lbm.resolved_schedule() == "handover"
    lbm.LBM_timestep(1)
    ref.timestep()
    _compare(lbm, ref, f"{dims} tau={tau} hand-over step 1")
    lbm.LBM_timestep(STEPS - 1)
    for _ in range(STEPS - 1):
        ref.timestep()
    f, g = lbm.populations()
    assert np.abs(f - ref.f).max() <= 1e-13 and np.abs(g - ref.g).max() <= 1e-13
    lbm.close()


@pytest.mark.parametrize("schedule", EXACT)
def test_batch_of_unit_rate_replicas_and_a_mixed_batch(pkg, ob, schedule):
    """All replicas at tau = 1/2: the batch's unit-rate kernels.  One replica at another tau: the generic ones.  Every replica
    equals the oracle either way."""
    n = (40, 24, 20)
    for taus in ((0.5, 0.5, 0.5), (0.5, 0.7, 0.5)):
        params = [dict(alpha0=1.5 + 0.25 * r, rho_lo=0.0, tau_f=t, tau_g=t) for r, t in enumerate(taus)]
        with pkg.BatchLBM(n, params=params, schedule=schedule) as b:
            refs = []
            for r, p in enumerate(params):
                b.replicas[r].LBM_init_droplet(0.2 + 0.05 * r)
                ref = ob.OracleLattice(*n, params=ob.default_params(**p))
                ref.init_droplet(0.2 + 0.05 * r)
                refs.append(ref)
            b.LBM_timestep(STEPS)
            for r, ref in enumerate(refs):
                for _ in range(STEPS):
                    ref.timestep()
                _compare(b.replicas[r], ref, f"batch {taus} replica {r} {schedule}")
