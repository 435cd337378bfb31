"""GPU: lag traces (LagTrace, bflbm_lag_*): two-time correlations of chosen hydrodynamic variables against time origins kept
on the device, and the persistence of the side of a level.

The rule and the order of the sums are in include/bflbm.h ("Lag traces"); analysis.lag_record restates them in numpy and
tests/test_lag_abi.py holds that twin to a plain per-origin loop.  Here the device record is compared with the twin of the
frames downloaded between the steps of the same run, bit for bit: lone lattices and replicas of a batch, the mixture of
tests/test_gpu_ring_recorders.py at kBT = 1e-5, 8 samples each."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

MIXTURE = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0)      # tests/test_gpu_ring_recorders.MIXTURE
SAMPLES = 8
HYD8 = [0, 1, 2, 3, 4, 9, 12, 21]                          # rho phi ufx ufy ufz afx agx ugbarx
BAR8 = [0, 1, 2, 3, 4, 5, 6, 7]
PAIRS8 = [(k, (3 * k + 1) % 8) for k in range(8)]          # a != b throughout ...
PAIRS8[3] = (3, 3)                                         # ... but one
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lag_mixture.npz")

# (box, source, variables, pairs, R, E, every, persist variable or None)
CASES = [
    ((33, 7, 5), "hydrovs", ["phi"], [("phi", "phi")], 1, 1, 1, "phi"),
    ((33, 7, 5), "hydrovs", ["rho", "phi", "ufx"], [("rho", "phi"), ("ufx", "ufx"), ("phi", "rho")], 3, 2, 3, "phi"),
    ((33, 7, 5), "hydrovsbar", BAR8, PAIRS8, 16, 1, 1, None),
    ((64, 32, 3), "hydrovs", HYD8, PAIRS8, 3, 2, 1, 1),
    ((64, 32, 3), "hydrovsbar", ["phi"], ["phi"], 16, 1, 3, "phi"),
    ((64, 32, 3), "hydrovs", ["ubx", "uby", "ubz"], ["ubx", "uby", "ubz"], 1, 1, 1, None),
    ((70, 33, 4), "hydrovs", ["rho", "phi", "ufx"], [("phi", "phi"), ("rho", "ufx")], 16, 1, 3, "phi"),
    ((70, 33, 4), "hydrovsbar", ["rho", "phi", "ufx"], [("rho", "rho"), ("ufx", "phi")], 3, 2, 1, None),
    ((70, 33, 4), "hydrovs", ["ubx"], ["ubx"], 3, 2, 3, None),
    ((70, 33, 4), "hydrovs", HYD8, PAIRS8, 1, 1, 3, 1),
]


def _case_id(c):
    return "%dx%dx%d-%s-nv%d-R%dE%d-every%d-%s" % (c[0] + (c[1], len(c[2]), c[4], c[5], c[6], "persist" if c[7] is not None else "plain"))


def _mixture(pkg, n, schedule=None, **params):
    p = dict(MIXTURE)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_mixture()
    return lbm


def _components(pkg, source, variables):
    names = pkg.plotfile.variable_names(9 if source == "hydrovsbar" else 22)
    return [names.index(v) if isinstance(v, str) else int(v) for v in variables]


def _slot_pairs(variables, pairs):
    slot = lambda v: variables.index(v) if isinstance(v, str) else int(v)
    return [(slot(p), slot(p)) if isinstance(p, str) else (slot(p[0]), slot(p[1])) for p in pairs]


def _frame(pkg, lattice, source, variables):
    fields = lattice.LBM_hydrovars_density() if source == "hydrovsbar" else lattice.LBM_hydrovars()
    return fields[_components(pkg, source, variables)].copy()


def _run(pkg, owner, lattices, source, variables, pairs, r, e, every, persist, samples=SAMPLES, level=None, capacity=SAMPLES):
    """Steps the owner `every` steps at a time and downloads the frames of every lattice in between.  The trace is made
    after the first frame, whose median gives the persistence level, and takes that frame by hand as sample 0; the other
    samples are the owner's.  Returns (trace, frames[lattice][sample], steps[lattice][sample], level)."""
    frames, steps = [[] for _ in lattices], [[] for _ in lattices]
    tr = None
    for k in range(samples):
        owner.LBM_timestep(every)
        for i, v in enumerate(lattices):
            frames[i].append(_frame(pkg, v, source, variables))
            steps[i].append(v.steps_done)
        if k == 0:
            if persist is not None and level is None:
                slot = variables.index(persist) if isinstance(persist, str) else persist
                level = float(np.median(frames[0][0][slot]))
            tr = owner.lag_trace(variables, pairs, origins=r, origin_stride=e, persist=None if persist is None else (persist, level),
                                 source=source, every=every, capacity=capacity)
            tr.sample()
    return tr, [np.array(f) for f in frames], [np.array(s, dtype=np.int64) for s in steps], level


def _twin(pkg, frames, steps, variables, pairs, r, e, persist, level):
    slot = -1 if persist is None else (variables.index(persist) if isinstance(persist, str) else persist)
    return pkg.analysis.lag_record(frames, steps, _slot_pairs(variables, pairs), r, e, slot, 0.0 if level is None else level)


def _assert_not_vacuous(pkg, want, r, e, nsites):
    """A condition on the inputs, not on the code under test: at every lag > 0 some sites have crossed and some have not."""
    held = pkg.analysis.lag_slots(len(want[0]), r, e)
    later = (held >= 0) & (held != np.arange(len(held))[:, None])
    alive = want[2]
    assert ((alive[later] > 0) & (alive[later] < nsites)).all(), alive
    assert (alive[held == np.arange(len(held))[:, None]] == nsites).all()
    return alive[later]


def _assert_equal(got, want, k=0):
    """The device record of replica k against the twin: the integers and the doubles alike, NaN for NaN in the empty slots."""
    steps, now, osteps, alive, corr = got
    assert osteps.dtype == np.int64 and alive.dtype == np.int64 and now.dtype == np.float64 and corr.dtype == np.float64
    assert np.array_equal(osteps[:, k], want[1]), (osteps[:, k], want[1])
    assert np.array_equal(alive[:, k], want[2]), (alive[:, k], want[2])
    assert np.array_equal(now[:, k], want[0]), np.abs(now[:, k] - want[0]).max()
    assert np.array_equal(np.isnan(corr[:, k]), np.isnan(want[3]))
    assert np.array_equal(corr[:, k], want[3], equal_nan=True), np.nanmax(np.abs(corr[:, k] - want[3]))


# ---- 1. against the definition, and 5. persistence is not vacuous -------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_lone_record_equals_the_twin(pkg, case):
    n, source, variables, pairs, r, e, every, persist = case
    nsites = n[0] * n[1] * n[2]
    lbm = _mixture(pkg, n)
    tr, frames, steps, level = _run(pkg, lbm, [lbm], source, variables, pairs, r, e, every, persist)
    want = _twin(pkg, frames[0], steps[0], variables, pairs, r, e, persist, level)
    if persist is not None:
        later = _assert_not_vacuous(pkg, want, r, e, nsites)
        print("%s: level %.17g, alive at the lags > 0: %s of %d" % (_case_id(case), level, sorted(set(later.tolist()), reverse=True), nsites))
    got = tr.read()
    assert got[0][:, 0].tolist() == [every * (k + 1) for k in range(SAMPLES)] and got[0].dtype == np.int64
    nv, npairs = len(variables), len(pairs)
    assert got[1].shape == (SAMPLES, 1, nv) and got[2].shape == (SAMPLES, 1, r) and got[3].shape == (SAMPLES, 1, r) and got[4].shape == (SAMPLES, 1, r, npairs)
    _assert_equal(got, want)
    held = pkg.analysis.lag_slots(SAMPLES, r, e)
    assert np.array_equal(got[2][:, 0] < 0, held < 0) and ((held[-1] < 0).any() == (r > (SAMPLES - 1) // e + 1))      # empty slots where the schedule leaves them
    assert np.ptp(got[1][:, 0, 0]) > 0 or variables == ["rho"]            # the state moves between the samples
    geo = tr.geometry()
    assert geo[:7] == (nv, npairs, r, e, nv + r * (2 + npairs), 2048, -(-n[0] * n[1] // 2048))
    assert geo[7:] == (8 * r * nv * nsites, 2 * nsites if persist is not None else 0)
    assert tr.names == [pkg.plotfile.variable_names(22)[c] for c in _components(pkg, source, variables)]
    lbm.close()


# ---- 2. the fixture of the CPU oracle ----------------------------------------------------------------------------------------
def test_fused_record_equals_the_oracle_fixture(pkg):
    """(70, 33, 4) under the fused schedule against tests/golden/lag_mixture.npz (make_golden_lag.py): the twin applied to
    the CPU oracle's frames."""
    import make_golden_lag as mg
    golden = np.load(GOLDEN)
    lbm = _mixture(pkg, mg.SHAPE, schedule="fused")
    assert lbm.resolved_schedule() == "fused"
    tr, frames, steps, level = _run(pkg, lbm, [lbm], "hydrovs", mg.VARIABLES, mg.PAIRS, mg.R, mg.E, mg.EVERY, mg.PERSIST, level=float(golden["level"]))
    got = tr.read()
    assert np.array_equal(got[0][:, 0], golden["steps"])
    _assert_equal(got, (golden["now"], golden["origin_steps"], golden["alive"], golden["corr"]))
    assert float(np.median(frames[0][0][mg.VARIABLES.index(mg.PERSIST)])) == float(golden["level"])
    lbm.close()


# ---- 3. batches --------------------------------------------------------------------------------------------------------------
BATCH_BOX = (16, 8, 8)
BATCH_VARS, BATCH_PAIRS = ["rho", "phi", "ufz"], [("phi", "phi"), ("ufz", "rho")]
BATCH_R, BATCH_E, BATCH_EVERY = 3, 2, 3


def _batch_params(count=3):
    return [dict(MIXTURE, alpha0=a, seed=s) for a, s in zip((1.0, 0.5, 1.5, 0.75, 1.25)[:count], (101, 202, 303, 404, 505)[:count])]


def _batch(pkg, params):
    batch = pkg.BatchLBM(BATCH_BOX, params=params)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    return batch


def test_batch_record_equals_the_twin_the_lone_lattice_and_a_larger_batch(pkg):
    nsites = BATCH_BOX[0] * BATCH_BOX[1] * BATCH_BOX[2]
    batch = _batch(pkg, _batch_params())
    tr, frames, steps, level = _run(pkg, batch, batch.replicas, "hydrovs", BATCH_VARS, BATCH_PAIRS, BATCH_R, BATCH_E, BATCH_EVERY, "phi")
    got = [np.array(v) for v in tr.read()]
    assert tr.geometry() == (3, 2, 3, 2, 15, 2048, 1, 221184, 6144)       # the figures tests/lag_main.cpp holds the host part to
    assert got[0][:, 1].tolist() == [1000 + 3 * (k + 1) for k in range(SAMPLES)] and got[0][:, 0].tolist() == [3 * (k + 1) for k in range(SAMPLES)]
    for k in range(3):
        want = _twin(pkg, frames[k], steps[k], BATCH_VARS, BATCH_PAIRS, BATCH_R, BATCH_E, "phi", level)
        later = _assert_not_vacuous(pkg, want, BATCH_R, BATCH_E, nsites)
        print("replica %d: alive at the lags > 0: %s of %d" % (k, sorted(set(later.tolist()), reverse=True), nsites))
        _assert_equal(got, want, k)
    assert got[2][0, 1, 0] == 1003 and not np.array_equal(got[4][:, 0], got[4][:, 1])          # each replica's own counter; they differ
    batch.close()
    for k, p in enumerate(_batch_params()):                # every replica run alone
        lbm = _mixture(pkg, BATCH_BOX, **p)
        if k == 1:
            lbm.set_steps_done(1000)
        alone = _run(pkg, lbm, [lbm], "hydrovs", BATCH_VARS, BATCH_PAIRS, BATCH_R, BATCH_E, BATCH_EVERY, "phi", level=level)[0].read()
        for u, v in zip(alone, got):
            assert np.array_equal(u[:, 0], v[:, k], equal_nan=True), k
        lbm.close()
    five = _batch(pkg, _batch_params(5))                   # the same replicas inside a batch of 5
    wide = _run(pkg, five, five.replicas, "hydrovs", BATCH_VARS, BATCH_PAIRS, BATCH_R, BATCH_E, BATCH_EVERY, "phi", level=level)[0].read()
    for u, v in zip(wide, got):
        assert np.array_equal(u[:, :3], v, equal_nan=True)
    five.close()


# ---- 4. the profile trace of the same owner ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(33, 7, 5), (70, 33, 4)])
def test_now_and_lag_zero_equal_the_profile_trace_summed_over_z(pkg, n):
    variables, pairs = ["rho", "phi", "ufx"], [("rho", "phi"), ("ufx", "ufx")]
    lbm = _mixture(pkg, n)
    prof = lbm.profile_trace(variables, pairs, axis="z", every=2, capacity=SAMPLES)
    tr = lbm.lag_trace(variables, pairs, origins=3, origin_stride=2, every=2, capacity=SAMPLES)
    lbm.LBM_timestep(2 * SAMPLES)
    sums, psteps = prof.read()                             # [count, 1, Q, nz]
    steps, now, osteps, alive, corr = tr.read()
    assert np.array_equal(psteps, steps) and (alive == -1).all()
    total = np.zeros(sums.shape[:3])
    for z in range(n[2]):                                  # the planes in sequence, from +0.0
        total = total + sums[..., z]
    assert np.array_equal(now[:, 0], total[:, 0, :3])
    fresh = osteps[:, 0] == steps                          # [count, R]: the origins at lag 0
    assert fresh.sum() == SAMPLES // 2 and (fresh.sum(axis=1) == [1, 0] * (SAMPLES // 2)).all()
    for k, r in zip(*np.nonzero(fresh)):
        assert np.array_equal(corr[k, 0, r], total[k, 0, 3:]), (k, r)
    lbm.close()


# ---- 6. lifecycle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_sample_reset_windows_overflow_and_detach(pkg, owner):
    n = BATCH_BOX
    nsites = n[0] * n[1] * n[2]
    o = _mixture(pkg, n) if owner == "lone" else _batch(pkg, _batch_params())
    first = o if owner == "lone" else o.replicas[0]
    tr = o.lag_trace(["phi"], ["phi"], origins=2, origin_stride=1, persist=("phi", 1.0), every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="lag trace full"):
        o.LBM_timestep(8)
    assert first.steps_done == 0 and tr.count == 0         # refused whole: nothing stepped, nothing recorded
    tr.sample()                                            # frame 0 by hand: origin 0
    tr.sample()                                            # twice on the same state: origin 1 equals origin 0
    steps, now, osteps, alive, corr = tr.read()
    assert tr.count == 2 and steps[:, 0].tolist() == [0, 0] and osteps[:, 0].tolist() == [[0, -1], [0, 0]]
    assert alive[:, 0].tolist() == [[nsites, -1], [nsites, nsites]] and corr[1, 0, 0, 0] == corr[1, 0, 1, 0] == corr[0, 0, 0, 0]
    assert np.isnan(corr[0, 0, 1, 0]) and np.array_equal(now[0], now[1])
    tr.reset()                                             # empties the slots and restarts n
    assert tr.count == 0 and tr.read()[1].shape == (0, steps.shape[1], 1)
    o.LBM_timestep(2)                                      # sample 0 after step 2
    steps, now, osteps, alive, corr = tr.read()
    assert steps[:, 0].tolist() == [2] and osteps[0, 0].tolist() == [2, -1] and alive[0, 0].tolist() == [nsites, -1] and np.isnan(corr[0, 0, 1, 0])
    tr.sample()                                            # by hand on the same state: the every-count does not move
    o.LBM_timestep(2)
    assert tr.count == 3 and first.steps_done == 4
    full = [np.array(v) for v in tr.read()]
    assert full[0][:, 0].tolist() == [2, 2, 4] and full[2][:, 0].tolist() == [[2, -1], [2, 2], [4, 2]]          # sample 2 overwrote slot 0
    assert full[3][2, 0, 0] == nsites and 0 < full[3][2, 0, 1] <= nsites
    frame = _frame(pkg, first, "hydrovs", ["phi"])
    assert full[3][2, 0, 1] <= np.count_nonzero(frame[0] >= 1.0) + np.count_nonzero(frame[0] < 1.0)
    with pytest.raises(pkg.BflbmError, match="lag trace full"):
        o.LBM_timestep(2)
    with pytest.raises(pkg.BflbmError, match="lag trace full"):
        tr.sample()
    assert first.steps_done == 4 and tr.count == 3
    window = tr.read(first=1, count=2)                     # a window of the record
    for u, v in zip(window, full):
        assert np.array_equal(u, v[1:], equal_nan=True)
    lags, mean, count = tr.correlation("phi")
    assert lags.tolist() == [0, 2] and count.tolist() == [4, 1]       # lag 0: both slots at the hand sample of step 2
    assert mean[0] == full[4][[0, 1, 1, 2], 0, [0, 0, 1, 0], 0].mean() and mean[1] == full[4][2, 0, 1, 0]
    plags, pmean, pcount = tr.persistence()
    assert plags.tolist() == [0, 2] and pmean[0] == 1.0 and pmean[1] == full[3][2, 0, 1] / nsites
    clags, cmean, ccount = tr.correlation(("phi", "phi"), connected=True)
    assert clags.tolist() == [0, 2] and 0 < cmean[0] < 1e-2 * mean[0]           # nsites x the variance of phi, against nsites x its square
    geo = tr.geometry()
    o.close()                                              # the owner goes first: the trace stays readable with the same bits
    assert tr._h is not None and tr.geometry() == geo
    for u, v in zip(tr.read(), full):
        assert np.array_equal(u, v, equal_nan=True)
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (10, 6, 13)
    lbm, batch = _mixture(pkg, n), pkg.BatchLBM(n, params=_batch_params())
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_lag_create.*replica of a batch.*use bflbm_batch_lag_create"):
        batch.replicas[0].lag_trace(["rho"], ["rho"])
    for owner, call in ((lbm, "bflbm_lag_create"), (batch, "bflbm_batch_lag_create")):
        nrep = 3 if owner is batch else 1
        for pattern, variables, pairs, kw in (("variable index 22 outside hydrovs", [0, 22], [(0, 0)], {}),
                                              ("variable index 9 outside hydrovsbar", [9], [(0, 0)], dict(source="hydrovsbar")),
                                              ("variable index 3 given twice", [3, 1, 3], [(0, 0)], {}),
                                              ("1..8 variables", list(range(9)), [(0, 0)], {}),
                                              (r"1..8 pairs \(got 0\)", [0], [], {}),
                                              (r"1..8 pairs \(got 9\)", [0], [(0, 0)] * 9, {}),
                                              ("pair 1: slot 2 outside the 2 variables", [0, 1], [(0, 1), (2, 0)], {}),
                                              (r"1..16 origins \(got 0\)", [0], [(0, 0)], dict(origins=0)),
                                              (r"1..16 origins \(got 17\)", [0], [(0, 0)], dict(origins=17)),
                                              (r"origin_stride must be >= 1 \(got 0\)", [0], [(0, 0)], dict(origin_stride=0)),
                                              (r"persist_slot 1 outside -1..0", [0], [(0, 0)], dict(persist=(1, 0.5))),
                                              (r"persist_slot -2 outside -1..0", [0], [(0, 0)], dict(persist=(-2, 0.5))),
                                              (r"persist_level must be finite \(got nan\)", [0], [(0, 0)], dict(persist=(0, float("nan")))),
                                              (r"persist_level must be finite \(got inf\)", [0], [(0, 0)], dict(persist=(0, float("inf")))),
                                              ("every must be >= 1", [0], [(0, 0)], dict(every=0)),
                                              ("capacity must be >= 1", [0], [(0, 0)], dict(capacity=0)),
                                              ("exceeds 1 TB", [0], [(0, 0)], dict(origins=1, capacity=(1 << 37) // (4 * nrep) + 1))):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                owner.lag_trace(variables, pairs, **kw)
            assert call in str(e.value), (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
    for bad in (lambda: lbm.lag_trace(["no_such_variable"], [(0, 0)]), lambda: lbm.lag_trace(["rho"], [("phi", "rho")]),
                lambda: lbm.lag_trace(["rho"], ["rho"], source="noise"), lambda: lbm.lag_trace(["rho"], ["rho"], persist=("phi", 0.0)),
                lambda: lbm.lag_trace(["rho"], ["rho"], persist=0.5)):
        with pytest.raises(ValueError):
            bad()
    tr = lbm.lag_trace(["rho"], ["rho"], capacity=2)
    for bad in (lambda: tr.correlation(1), lambda: tr.correlation(("rho", "phi")), tr.persistence):
        with pytest.raises(ValueError):
            bad()
    tr.close()
    assert not hasattr(pkg.RingLBM, "lag_trace")
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_lag_create inside an open step"):
        lbm.lag_trace(["rho"], ["rho"])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.lag_trace(["rho"], ["rho"], capacity=2)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [1, 2]       # the split step samples in its finish
    lbm.close(); batch.close()
    # a slab of a decomposed lattice handed to the lone call
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_lag_create.*nranks > 1"):
        slab.lag_trace(["rho"], ["rho"])
    slab.close()


# ---- a recorder changes nothing ----------------------------------------------------------------------------------------------
def test_a_lag_trace_changes_nothing(pkg):
    n = (12, 10, 14)
    a, b = _mixture(pkg, n, "fused"), _mixture(pkg, n, "fused")
    tr = a.lag_trace(["phi", "ufx"], [("phi", "phi"), ("ufx", "phi")], origins=4, origin_stride=2, persist=("phi", 1.0), every=1, capacity=13)
    other = a.histogram_trace({"phi": (0.9, 1.1, 16)}, every=1, capacity=13)
    a.LBM_timestep(12); b.LBM_timestep(12)
    assert tr.count == 12 and other.count == 12
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    a.LBM_timestep(1); b.LBM_timestep(1)                   # the step after the last sample
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    a.close(); b.close()
