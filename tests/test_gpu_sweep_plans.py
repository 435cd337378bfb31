"""GPU: the plane-marching sweeps under the launch plans of LARGE lattices, against the CPU oracle.

tests/test_gpu_handover_oracle.py runs the default kernel (k_fused_ho, its _unit, noise and ragged forms) on lattices that
the chunk planner always cuts into chunks of 4 to 6 planes in one round (tests/test_sweep_plans.py pins that): 7 march
positions, at most 3 planes per chunk that read frames, hardly any steady state.  Here the smallest lattices that get the
plans of 256^3, 512^3, 320^3 and of the slabs of a large ring (tests/sweep_plan_cases.py):
  long    one chunk of 40 planes, exactly 256 workgroups;         rounds  ntx = 8, one chunk of 24, 2 rounds;
  cut     chunks of 9, 9, 8 in 4 rounds, padded grid;             cut7    ntx = 7, three chunks of 11;
  ring    2 slabs whose interior sweep is ONE chunk of 8 planes in 3 rounds, boundary pairs in one launch;
the ragged twins of long, rounds and ring have a last tile column of 58 / 52 lanes and a last tile row of 2 rows.
Every case first asserts, through the library's own planner (sweep_plan_query with the device's compute units), that it
runs under the plan of the table -- it fails, it does not skip, on a device the table was not chosen for.

Input: the oracle's stripe at alpha0 = 2, rho_lo = 0.1 with every population multiplied by 1 + 0.01 N(0, 1), uploaded into
both sides: no two tiles alike (a frame taken from the wrong tile shows), no site near vacuum.  The oracle answers a
one-ulp change of this input (tolerances.one_ulp_response; measured at (128, 16, 24) and (64, 12, 40) after 2 and 8 steps,
for the three parameter sets below) with 7e-16 ... 1.0e-15 relative in the densities and 1.5e-16 ... 3.9e-16 cs in the
velocities, the minimum density staying at 0.087: three orders inside the strict 1e-12 form, which is therefore asserted
outright -- no case here may be added to tests/golden/handover_strict_exceptions.json.

Per hand-over case, with one step per call and checkpoints at steps 1, 2 and the last (6; the ring 4):
  step 1   populations, hydrovars and (noise) thermal_noise() equal the oracle's bit for bit;
  step 2   the first step that reads frames.  The streaming shift of both downloads is undone (post-collision
           S_i(x) = f_i(x + c_i), exact on a periodic lattice); the sites where S differs from the oracle's must be
           (b) tile-edge sites -- x the first or last active column of a 64-wide tile, y the first or last active row of
           a 4-high one: only their gradient stencil reaches ring sites -- on
           (a) planes whose stencil reaches a plane whose ring came from frames.  A chunk [qa, qb) takes the ring
           densities of the planes qa+1 ... qb-2 from frames (bflbm_handover_body.inc:101-102 `fa = qa + 1, fb = qb - 2`,
           used at :164 and :207) -- the planes strictly inside it -- and pulls those of qa-1, qa, qb-1, qb; the stencil
           of plane p reads p-1, p, p+1, so in a chunk of at least 3 planes EVERY plane qa ... qb-1 may differ, and each
           of them must (thousands of edge sites per plane, each a re-ordered sum of 19 numbers: a plane without any
           ran the pulled path).  The 2-plane chunks of a slab's boundary pairs frame nothing (fa > fb): those planes
           are bit-equal.
           Everything outside (a) x (b) is bit-equal: a difference there is a frame read for the wrong plane, tile or
           role, or a changed own-site sum, however small.
  every checkpoint   populations within 1e-13 of the oracle's (the bound of test_gpu_handover_oracle.py);
  last     tolerances.check at 1e-12 and the strict form, asserted;
  then     a fresh lattice takes the same steps in ONE call: the same bits (frame signatures across calls).
The exact schedules -- "fused" at tau = 1/2 (k_fused_unit) and at (0.8, 0.6) (k_fused), "two_pass" with noise -- run the
lone shapes of the one-pass table and the ring, bit for bit at every checkpoint.
One oracle trajectory per (shape, parameter set) serves every schedule; one is kept at a time, as is one lattice."""
import numpy as np
import pytest

import sweep_plan_cases as sp
import tolerances

pytestmark = pytest.mark.gpu

BASE = dict(alpha0=2.0, rho_lo=0.1)
FORMS = {
    "unit": dict(),                                      # tau = 1/2: k_fused_ho_unit, full and ragged
    "generic": dict(tau_f=0.8, tau_g=0.6),               # k_fused_ho<4, 0, *>
    "noise": dict(kBT=1e-5, alpha0=1.0, tau_f=0.8),      # k_fused_ho<4, 1, *>
}
EXACT = {"unit": "fused", "generic": "fused", "noise": "two_pass"}
LONE_STEPS, RING_STEPS = (1, 2, 6), (1, 2, 4)
MIN_DENSITY = 0.05                                       # "no site near vacuum": measured 0.087, rho_lo = 0.1

# (case, form, schedule), the users of one trajectory next to each other
CASES = []
for _case in ("long", "rounds", "cut"):
    for _form in FORMS:
        CASES += [(_case, _form, "handover"), (_case, _form, EXACT[_form])]
for _case in ("cut7",):
    CASES += [(_case, _form, "handover") for _form in FORMS]
for _case in ("long_ragged", "rounds_ragged"):
    CASES += [(_case, _form, "handover") for _form in ("unit", "noise")]
CASES += [("ring", "unit", "handover"), ("ring", "unit", "fused"), ("ring", "noise", "handover"),
          ("ring_ragged", "unit", "handover"), ("ring_ragged", "noise", "handover")]


@pytest.fixture()
def threads(ob):
    ob.lib().orc_set_threads(16)
    yield
    ob.lib().orc_set_threads(1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _table(case):
    return sp.RING[case] if case in sp.RING else sp.HANDOVER[case]


_TRAJECTORY = {}          # at most one entry: (shape, form) -> the oracle's run


def _trajectory(ob, shape, form, checkpoints):
    """The oracle's run from the perturbed stripe: the upload and, per checkpoint, populations (all), hydrovars and noise
    (first and last).  Read-only for its users."""
    key = (shape, form, checkpoints)
    if key not in _TRAJECTORY:
        _TRAJECTORY.clear()
        par = dict(BASE, **FORMS[form])
        ref = ob.OracleLattice(*shape, params=ob.default_params(**par))
        ref.init_stripe(0.5)
        rng = np.random.default_rng(20240611)
        f0 = np.ascontiguousarray(ref.f * (1.0 + 0.01 * rng.standard_normal(ref.f.shape)))
        g0 = np.ascontiguousarray(ref.g * (1.0 + 0.01 * rng.standard_normal(ref.g.shape)))
        ref.init_from(f0, g0)
        t = dict(par=par, f0=f0, g0=g0, at={})
        for steps in range(1, checkpoints[-1] + 1):
            ref.timestep()
            if steps in checkpoints:
                at = dict(f=ref.f.copy(), g=ref.g.copy())
                assert np.isfinite(at["f"]).all() and np.isfinite(at["g"]).all()
                assert min(ref.h[0].min(), ref.h[1].min()) >= MIN_DENSITY, f"{shape} {form} step {steps}: a site near vacuum"
                if steps in (checkpoints[0], checkpoints[-1]):
                    at.update(h=ref.h.copy(), fn=ref.fn.copy(), gn=ref.gn.copy())
                t["at"][steps] = at
        for a in (f0, g0, *[v for at in t["at"].values() for v in at.values()]):
            a.setflags(write=False)
        _TRAJECTORY[key] = t
    return _TRAJECTORY[key]


def _make(pkg, shape, par, ring, schedule):
    p = pkg.default_params(**par)
    if ring:
        lbm = pkg.RingLBM(*shape, nslabs=sp.NSLABS, params=p, schedule=schedule)
        assert [s.resolved_schedule() for s in lbm.slabs] == [schedule] * sp.NSLABS
        return lbm
    lbm = pkg.BinaryLBM(*shape, params=p, schedule=schedule)
    assert lbm.resolved_schedule() == schedule
    return lbm


def _plan_on_this_device(pkg, case, schedule, noise):
    """The plan the resident lattice runs under, from the planner with the device's compute units; it must be the table's."""
    ring = case in sp.RING
    if schedule == "two_pass":
        return None
    plan = pkg.sweep_plan_query(_table(case)["n"], schedule, noise=noise, slab_planes=sp.SLAB_PLANES if ring else 0, compute_units=0)
    assert plan["compute_units"] == sp.CUS, \
        f"the device reports {plan['compute_units']} compute units; the case table of sweep_plan_cases.py was chosen for {sp.CUS}"
    if schedule == "handover":
        (sp.check_ring if ring else sp.check_handover)(plan, case)
    elif ring:
        sp.check_fused_ring(plan)
    else:
        sp.check_fused(plan, case)
    return plan


def handover_chunks(case, plan):
    """[(qa, qb)] in lattice planes: the chunks of the plan whose ring densities can come from frames."""
    if case in sp.RING:                                  # every slab: its interior sweep starts behind the first boundary pair
        return [(s * sp.SLAB_PLANES + a, s * sp.SLAB_PLANES + b) for s in range(sp.NSLABS) for a, b in sp.chunk_ranges(plan, first=2)]
    return sp.chunk_ranges(plan)


def planes_that_may_differ(qa, qb):
    """bflbm_handover_body.inc:101-102: ring densities of the planes [qa+1, qb-2] come from frames; a collided plane p of
    the chunk reads the densities of p-1, p, p+1."""
    framed = set(range(qa + 1, qb - 1))
    return [p for p in range(qa, qb) if framed & {p - 1, p, p + 1}]


def edge_sites(case):
    """(ny, nx) mask of the tile-edge sites of the 64 x 4 tiling: first / last ACTIVE column or row of a tile."""
    t = _table(case)
    nx, ny, _ = t["n"]
    x, y = np.arange(nx), np.arange(ny)
    assert (nx - 1) % 64 == t["last_cols"] - 1 and (ny - 1) % 4 == t["last_row"] - 1
    ex = (x % 64 == 0) | (x % 64 == 63) | (x == nx - 1)
    ey = (y % 4 == 0) | (y % 4 == 3) | (y == ny - 1)
    return ey[:, None] | ex[None, :]


def post_collision_differences(f, g, rf, rg, c):
    """(nz, ny, nx) mask of the sites whose post-collision populations (either fluid, any direction) differ in any bit:
    stream_push wrote fnew_i(x + c_i) = S_i(x) (LBM_binary.H:519-531), so S_i(x) = f_i(x + c_i)."""
    out = np.zeros(f.shape[1:], dtype=bool)
    for i in range(f.shape[0]):
        bad = (_bits(f[i]) != _bits(rf[i])) | (_bits(g[i]) != _bits(rg[i]))
        if bad.any():
            out |= np.roll(bad, (-int(c[i][2]), -int(c[i][1]), -int(c[i][0])), axis=(0, 1, 2))
    return out


def check_frame_step(case, plan, diff, what):
    """The step-2 assertion of the module docstring on the mask of differing sites."""
    chunks = handover_chunks(case, plan)
    allowed_plane = np.zeros(diff.shape[0], dtype=bool)
    for qa, qb in chunks:
        allowed_plane[planes_that_may_differ(qa, qb)] = True
    edge = edge_sites(case)
    per_plane = diff.sum(axis=(1, 2))
    counts = [int(per_plane[qa:qb].sum()) for qa, qb in chunks]
    print(f"[sweep plans] {what} step 2: differing sites per chunk {dict(zip(chunks, counts))} of {int(edge.sum())} edge sites per plane; "
          f"fewest on a framed plane {int(per_plane[allowed_plane].min()) if allowed_plane.any() else None}")
    off_plane = diff & ~allowed_plane[:, None, None]
    off_edge = diff & ~edge[None]
    lines = []
    for name, m in (("on a plane that reads no frame", off_plane), ("at a site that is no tile edge", off_edge)):
        if m.any():
            z, y, x = np.nonzero(m)
            lines.append(f"{m.sum()} differing sites {name}: planes {np.unique(z).tolist()[:40]}, first (z, y, x) "
                         f"{list(zip(z[:8].tolist(), y[:8].tolist(), x[:8].tolist()))}, tiles (ty, tx) {sorted(set(zip((y // 4).tolist(), (x // 64).tolist())))[:8]}")
    if lines:
        pytest.fail(f"{what} step 2, chunks {chunks}:\n" + "\n".join(lines), pytrace=False)
    for (qa, qb), n in zip(chunks, counts):
        may = planes_that_may_differ(qa, qb)
        if may:
            assert n > 0, f"{what} step 2: chunk [{qa}, {qb}) equals the oracle bit for bit: it ran the pulled path"
            same = [p for p in may if per_plane[p] == 0]
            assert not same, f"{what} step 2: planes {same} of chunk [{qa}, {qb}) equal the oracle bit for bit: they ran the pulled path"


def _same_bits(name, got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (f"{what}: {name}: {np.count_nonzero(bad)} of {bad.size} doubles differ, components {np.flatnonzero(bad.any(axis=(1, 2, 3))).tolist()}, "
                           f"z-planes {np.flatnonzero(bad.any(axis=(0, 2, 3))).tolist()}, largest {np.abs(got - want).max():.3e}")


def _exact_checkpoint(lbm, at, noise, what):
    f, g = lbm.populations()
    _same_bits("f", f, at["f"], what)
    _same_bits("g", g, at["g"], what)
    del f, g
    if "h" in at:
        h = lbm.LBM_hydrovars()
        assert np.array_equal(h, at["h"]), f"{what}: hydrovars differ, largest {np.abs(h - at['h']).max():.3e}"
        if noise:
            fn, gn = lbm.thermal_noise()
            _same_bits("fnoise", fn, at["fn"], what)
            _same_bits("gnoise", gn, at["gn"], what)
            assert np.abs(fn).max() > 1e-5, what + ": no noise"


@pytest.mark.parametrize("case,form,schedule", CASES, ids=["-".join(c) for c in CASES])
def test_sweeps_under_large_lattice_plans(pkg, ob, threads, case, form, schedule):
    ring = case in sp.RING
    shape = _table(case)["n"]
    checkpoints = RING_STEPS if ring else LONE_STEPS
    noise = form == "noise"
    t = _trajectory(ob, shape, form, checkpoints)
    what = f"{case} {shape} {form} {schedule}"
    c = ob.lattice_tables()[0]

    lbm = _make(pkg, shape, t["par"], ring, schedule)
    plan = _plan_on_this_device(pkg, case, schedule, noise)
    print(f"[sweep plans] {what}: plan {plan}")
    lbm.LBM_init(t["f0"], t["g0"])
    last = None
    for steps in range(1, checkpoints[-1] + 1):
        lbm.LBM_timestep(1)                                                # one step per call
        if steps not in checkpoints:
            continue
        at, here = t["at"][steps], f"{what} step {steps}"
        if schedule != "handover" or steps == 1:
            _exact_checkpoint(lbm, at, noise, here)                        # the exact schedules always; hand-over: its first step
            continue
        f, g = lbm.populations()
        worst = max(np.abs(f - at["f"]).max(), np.abs(g - at["g"]).max())
        print(f"[sweep plans] {here}: populations within {worst:.3e} of the oracle's")
        assert worst < 1e-13, f"{here}: populations {worst:.3e} from the oracle's"
        if steps == 2:
            check_frame_step(case, plan, post_collision_differences(f, g, at["f"], at["g"], c), what)
        if steps == checkpoints[-1]:
            h = lbm.LBM_hydrovars()
            e = tolerances.check(h, at["h"], here, 1e-12)
            print(f"[sweep plans] {here}: strict form: densities {e['dens_elem_all']:.3e} relative, velocities {e['vel_abs_all']:.3e} cs "
                  f"at every site; masked {max(e[k] for k in tolerances.MASKED):.3e}")
            assert tolerances.strict(e), f"{here}: the strict form (densities relative 1e-12, velocities 1e-12 cs at every site) is violated: {e}"
            assert not (np.array_equal(f, at["f"]) and np.array_equal(g, at["g"])), here + ": bit-equal to the oracle: no frame was read"
            last = (f, g)
            del h
        del f, g
    lbm.close()
    if schedule != "handover":
        return
    lbm = _make(pkg, shape, t["par"], ring, schedule)                      # the same steps in one call
    lbm.LBM_init(t["f0"], t["g0"])
    lbm.LBM_timestep(checkpoints[-1])
    f, g = lbm.populations()
    lbm.close()
    _same_bits("f", f, last[0], what + f": one call of {checkpoints[-1]} steps against {checkpoints[-1]} calls of one")
    _same_bits("g", g, last[1], what + f": one call of {checkpoints[-1]} steps against {checkpoints[-1]} calls of one")
