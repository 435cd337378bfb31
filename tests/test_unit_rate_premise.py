"""CPU, no GPU: the arithmetic premise of the unit-rate kernels (csrc/bflbm_site.h, d_relax_with<false, true>).

At tau = 1/2 the host derives inv_tau_bar = 1./(tau*(1. + 0.5/tau)) == 1.0 exactly, and the zero-noise relaxation of
LBM_binary.H:504-511 does, for the ghost modes k = 10..18, `R = inv_tau_bar*(0. - m[k]) + 0.; m[k] = m[k] + R`.  The
unit-rate kernels write the literal +0.0 there without reading m[k] and drop the multiplication for k < 10.

(a) the IEEE identities, in numpy float64 (numpy evaluates one operation at a time: nothing is contracted);
(b) the same on the reference's own arithmetic through the CPU oracle: which outputs of `populations` can see the sign
    of a zero ghost mode at all, and that the post-collision populations of one oracle step at tau = 1/2 carry ghost
    modes no larger than the rounding of the moments -> populations -> moments round trip."""
import numpy as np
import pytest

Q = 19
DBL_MAX = np.finfo(np.float64).max
TINY = np.finfo(np.float64).tiny           # smallest normal
SUB = np.float64(5e-324)                   # smallest subnormal


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _samples():
    rng = np.random.default_rng(20250116)
    mant = rng.uniform(1.0, 2.0, 20000)
    expo = rng.integers(-1000, 1000, 20000)
    rnd = np.ldexp(mant, expo) * rng.choice([-1.0, 1.0], 20000)
    special = np.array([0.0, -0.0, SUB, -SUB, 123 * SUB, -TINY / 2, TINY, -TINY, np.nextafter(TINY, 0.0),
                        DBL_MAX / 2, -DBL_MAX / 2, np.nextafter(DBL_MAX / 2, 0.0), np.nextafter(DBL_MAX / 2, np.inf),
                        1.0, -1.0, 1.0 / 3.0, -1e-300, 1e300])
    sub = rng.integers(1, 2**52, 2000).astype(np.uint64).view(np.float64) * rng.choice([-1.0, 1.0], 2000)   # subnormals
    near_max = (DBL_MAX / 2) * rng.uniform(0.5, 1.0, 2000) * rng.choice([-1.0, 1.0], 2000)
    x = np.concatenate([rnd, special, sub, near_max])
    assert np.isfinite(x).all()
    return x


def test_ghost_mode_relaxation_at_unit_rate_is_plus_zero():
    m = _samples()
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(over="raise", invalid="raise"):
        R = one * (zero - m) + zero
        out = m + R
    assert np.array_equal(_bits(out), np.zeros(m.size, dtype=np.uint64)), "a ghost mode did not relax to +0.0"


def test_multiplication_by_unit_rate_keeps_the_bits():
    x = _samples()
    with np.errstate(over="raise", invalid="raise"):
        y = np.float64(1.0) * x
    assert np.array_equal(_bits(y), _bits(x))
    # and on a difference as the kernel forms it, (mEq - m): 1.0*(a - b) has the bits of (a - b)
    a, b = x[:-1], x[1:]
    with np.errstate(over="ignore"):
        d = a - b
    keep = np.isfinite(d)
    assert np.array_equal(_bits(np.float64(1.0) * d[keep]), _bits(d[keep]))


def unit_rate(tau):
    """1/tau_bar as the host derives it (csrc/bflbm.hip derive(): tau_bar = tau*(1. + 0.5/tau), LBM_binary.H:504-508)."""
    tau = np.float64(tau)
    return np.float64(1.0) / (tau * (np.float64(1.0) + np.float64(0.5) / tau))


def nearest_tau_with_another_rate(direction):
    """The double nearest to 1/2 on one side whose derived rate is not exactly 1.0 (the kernels are chosen by the derived
    rate, not by tau: neighbours of 1/2 whose tau_bar rounds to 1.0 multiply by exactly 1.0 in the generic kernel too)."""
    t = np.float64(0.5)
    for _ in range(16):
        t = np.nextafter(t, direction)
        if unit_rate(t) != 1.0:
            return float(t)
    raise AssertionError("no double within 16 ulp of 1/2 has a rate other than 1.0")


def test_tau_one_half_gives_the_unit_rate_exactly():
    assert unit_rate(0.5) == 1.0 and _bits(unit_rate(0.5)) == _bits(np.float64(1.0))
    assert unit_rate(1.0) != 1.0 and unit_rate(0.8) != 1.0
    lo, hi = nearest_tau_with_another_rate(0.0), nearest_tau_with_another_rate(1.0)
    print("nearest tau below / above 1/2 with a rate other than 1.0: %r (%d ulp), %r (%d ulp)"
          % (lo, round((0.5 - lo) / np.spacing(0.25)), hi, round((hi - 0.5) / np.spacing(0.5))))
    assert unit_rate(lo) != 1.0 and unit_rate(hi) != 1.0


# ---- (b) on the reference's arithmetic ------------------------------------------------------------------------------

def test_which_populations_see_the_sign_of_a_zero_ghost_mode(ob):
    """populations(m) with ghost modes +0.0 against the same m[0..9] with ghost modes -0.0.  The ghost modes enter every
    output through sums, so the sign of a zero can only show in an output whose other terms are all zero.  Asserted:
    the VALUES never differ, and the bits differ only in outputs that are zero.  Consequence for the kernels: the
    `x + 0.0` additions that the literal +0.0 leaves behind are what turns a -0.0 partial sum into the +0.0 the generic
    kernel stores at an empty site, so the unit-rate kernels keep them, and the GPU tests compare sign bits on lattices
    with vacuum (tests/test_gpu_unit_rate.py)."""
    rng = np.random.default_rng(7)
    seen = np.zeros(Q, dtype=bool)
    cases = [rng.normal(size=10) for _ in range(200)]
    cases += [np.eye(10)[k] * s for k in range(10) for s in (1.0, -1.0, 1e-300, -5e-324)]       # a single live mode
    cases += [np.zeros(10), -np.zeros(10)]                                                         # vacuum
    for low in cases:
        mp = np.concatenate([low, np.zeros(9)])
        mm = np.concatenate([low, -np.zeros(9)])
        fp, fm = ob.populations(mp), ob.populations(mm)
        assert np.array_equal(fp, fm), "a zero ghost mode changed a VALUE"
        differ = _bits(fp) != _bits(fm)
        assert not (differ & (fp != 0.0)).any(), "the sign of a zero ghost mode reached a non-zero population"
        seen |= differ
    # vacuum: ghost modes +0.0 give +0.0 in all 19 outputs (what both the generic and the unit-rate kernel store there)
    vac = ob.populations(np.zeros(Q))
    assert np.array_equal(_bits(vac), np.zeros(Q, dtype=np.uint64))
    print("outputs that can see the sign of a zero ghost mode (only while their value is zero):", np.flatnonzero(seen).tolist())


def _post_collision(c, lat):
    """The populations the last oracle step's collide wrote, before its streaming: f*_i(x) = f_i(x + c_i)."""
    def unstream(a):
        return np.stack([np.roll(a[i], shift=(-c[i][2], -c[i][1], -c[i][0]), axis=(0, 1, 2)) for i in range(Q)])
    return unstream(lat.f), unstream(lat.g)


def _ulp_of_largest(p):
    a = np.abs(p).max()
    return float(np.spacing(a)) if a > 0 else 0.0


@pytest.mark.parametrize("case", ["stripe", "droplet_in_vacuum"])
def test_ghost_modes_after_one_oracle_step_are_rounding_only(ob, case):
    """One oracle step at tau = 1/2; the un-streamed populations re-analysed with `moments`.  The oracle relaxed the ghost
    modes with the generic expression and the run-time rate 1.0, so what `moments` finds there is the rounding of
    populations() followed by moments() and nothing else.  The bound is measured, not guessed: the same re-analysis of
    populations(m) with the site's own m[0..9] and EXACTLY zero ghost modes, in ulps of the site's largest population,
    maximised over the lattice.  Both figures are printed.  The droplet sits in a flat 130 x 17 x 5 box (LBM_init_droplet
    centres it at z = nx/2, outside the box), whose far sites hold populations that are exactly zero: real vacuum."""
    c = np.asarray(ob.lattice_tables()[0]).reshape(Q, 3)
    if case == "stripe":
        lat = ob.OracleLattice(12, 12, 12)
        lat.init_stripe(0.5)
    else:
        lat = ob.OracleLattice(130, 17, 5, ob.default_params(rho_lo=0.0))
        lat.init_droplet(0.2)
    assert lat.p.tau_f == 0.5 and lat.p.tau_g == 0.5
    lat.timestep()
    worst, control, vacuum_sites = 0.0, 0.0, 0
    for pops in _post_collision(c, lat):
        flat = pops.reshape(Q, -1)
        for s in range(flat.shape[1]):
            p = np.ascontiguousarray(flat[:, s])
            u = _ulp_of_largest(p)
            m = ob.moments(p)
            if u == 0.0:                               # vacuum: every population is zero, and so is every moment
                vacuum_sites += 1
                assert not m.any()
                continue
            worst = max(worst, float(np.abs(m[10:]).max()) / u)
            m0 = m.copy()
            m0[10:] = 0.0
            p0 = ob.populations(m0)
            control = max(control, float(np.abs(ob.moments(p0)[10:]).max()) / _ulp_of_largest(p0))
    print(f"{case}: largest ghost mode after one step {worst:.2f} ulp of the site's largest population; "
          f"control (exactly zero ghost modes re-analysed) {control:.2f} ulp; vacuum sites {vacuum_sites}")
    assert control > 0.0
    assert worst <= control, (worst, control)
    if case == "droplet_in_vacuum":
        assert vacuum_sites > 0, "the droplet case is meant to contain exact vacuum"
