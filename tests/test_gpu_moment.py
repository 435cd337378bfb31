"""GPU: moment traces (MomentTrace, bflbm_moment_*): the box sums of all 19 kinetic moments of both fluids, of their squares
and of the products of the two fluids' moments.

The definition and the order of the sums are in include/bflbm.h ("Moment traces"); analysis.moment_record restates them in
numpy and tests/test_moment_abi.py holds that twin to the oracle's transform, to an int64 computation and to a plain sum.
Here the device record is compared with the twin of the populations downloaded between the steps of the same run, bit for
bit: lone lattices under every schedule, replicas of a batch, and the CPU oracle's fixture.

The boxes are the smallest at which the tiling can go wrong: (33, 7, 5) a plane below one tile with odd nx against the
padded pitch, (64, 32, 3) a plane of exactly one tile, (70, 33, 4) a ragged second tile."""
import os
import sys

import numpy as np
import pytest

import moment_sums as ms

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

MIXTURE = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0)      # tests/test_gpu_ring_recorders.MIXTURE
BOXES = [(33, 7, 5), (64, 32, 3), (70, 33, 4)]
HANDOVER_BOX = (64, 8, 16)                                 # tests/test_gpu_shape.HANDOVER_SHAPE: the hand-over kernel does run here
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moment_mixture.npz")
STEPS = 4


def _mixture(pkg, n, schedule=None, **params):
    p = dict(MIXTURE)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_mixture()
    return lbm


def _twin(pkg, lattice):
    f, g = lattice.populations()
    return pkg.analysis.moment_record(f, g)


def _same(got, want):
    """Equal doubles; the message names the words that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:8].tolist(), np.abs(got - want).max())


# ---- 1. against the definition ---------------------------------------------------------------------------------------------
LONE_CASES = [(n, s, kBT) for n in BOXES for s in ("fused", "two_pass", "handover") for kBT in (0.0, 1e-5)]
LONE_CASES += [(HANDOVER_BOX, "handover", kBT) for kBT in (0.0, 1e-5)]


@pytest.mark.parametrize("n,schedule,kBT", LONE_CASES, ids=lambda v: "%dx%dx%d" % v if isinstance(v, tuple) else str(v))
def test_lone_record_equals_the_twin(pkg, n, schedule, kBT):
    """After 0 (by hand), 1, 2, 3 and 4 steps with every = 1, and after 0, 2 and 4 with every = 2, on one run.  The
    hand-over schedule is asked for on every box; on the small ones the library resolves it to a bit-exact schedule (printed)."""
    lbm = _mixture(pkg, n, schedule, kBT=kBT)
    if n == HANDOVER_BOX:
        assert lbm.resolved_schedule() == "handover"
    one, two = lbm.moment_trace(every=1, capacity=STEPS + 1), lbm.moment_trace(every=2, capacity=STEPS // 2 + 1)
    one.sample(); two.sample()
    want = [_twin(pkg, lbm)]
    for _ in range(STEPS):
        lbm.LBM_timestep(1)
        want.append(_twin(pkg, lbm))
    want = np.array(want)
    print("%s %s kBT %g: resolved %s" % (n, schedule, kBT, lbm.resolved_schedule()))
    steps, sums = one.read()
    assert steps.dtype == np.int64 and steps[:, 0].tolist() == list(range(STEPS + 1)) and sums.shape == (STEPS + 1, 1, 95)
    _same(sums[:, 0], want)
    steps2, sums2 = two.read()
    assert steps2[:, 0].tolist() == [0, 2, 4]
    _same(sums2[:, 0], want[::2])
    assert one.geometry() == (95, 2048, -(-n[0] * n[1] // 2048)) == two.geometry()
    _same(one.sums("f")[:, 0], want[:, :19]); _same(one.sums(1)[:, 0], want[:, 19:38])
    _same(one.squares(0)[:, 0], want[:, 38:57]); _same(one.squares("g")[:, 0], want[:, 57:76]); _same(one.cross()[:, 0], want[:, 76:])
    nsites = n[0] * n[1] * n[2]
    print("  rho_f %.6g rho_g %.6g per site; the record moves: %s" % (sums[0, 0, 0] / nsites, sums[0, 0, 19] / nsites, not np.array_equal(sums[0], sums[-1])))
    assert kBT == 0.0 or not np.array_equal(sums[1, 0, 38:], sums[-1, 0, 38:])      # with noise the squares move between the samples
    lbm.close()


# ---- 2. an integer state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES, ids=lambda n: "%dx%dx%d" % n)
def test_integer_state_equals_the_int64_computation(pkg, n):
    f0, g0 = ms.integer_populations((n[2], n[1], n[0]), seed=n[0])
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**MIXTURE))
    lbm.LBM_init(f0, g0)
    tr = lbm.moment_trace(capacity=1)
    tr.sample()
    steps, sums = tr.read()
    want = ms.integer_record(f0, g0)
    assert steps.tolist() == [[0]] and np.abs(want).max() < 2 ** 53
    _same(sums[0, 0], want.astype(np.float64))
    _same(sums[0, 0], pkg.analysis.moment_record(*lbm.populations()))
    lbm.close()


# ---- 3. batches --------------------------------------------------------------------------------------------------------------
BATCH_BOX = (70, 33, 4)


def _batch_params(count=3):
    return [dict(MIXTURE, alpha0=a, seed=s) for a, s in zip((1.0, 0.5, 1.5, 0.75, 1.25)[:count], (101, 202, 303, 404, 505)[:count])]


def _batch(pkg, params):
    batch = pkg.BatchLBM(BATCH_BOX, params=params)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    return batch


def _batch_run(pkg, owner, lattices):
    tr = owner.moment_trace(every=1, capacity=STEPS + 1)
    tr.sample()
    want = [[_twin(pkg, v) for v in lattices]]
    for _ in range(STEPS):
        owner.LBM_timestep(1)
        want.append([_twin(pkg, v) for v in lattices])
    return tr.read(), np.array(want)


def test_batch_record_equals_the_twin_the_lone_lattice_and_a_larger_batch(pkg):
    batch = _batch(pkg, _batch_params())
    (steps, sums), want = _batch_run(pkg, batch, batch.replicas)
    assert sums.shape == (STEPS + 1, 3, 95) and steps[:, 0].tolist() == list(range(STEPS + 1)) and steps[:, 1].tolist() == [1000 + k for k in range(STEPS + 1)]
    _same(sums, want)
    assert not np.array_equal(sums[:, 0], sums[:, 1]) and not np.array_equal(sums[:, 1], sums[:, 2])
    batch.close()
    for k, p in enumerate(_batch_params()):                # every replica run alone
        lbm = _mixture(pkg, BATCH_BOX, **p)
        if k == 1:
            lbm.set_steps_done(1000)
        (s1, alone), _ = _batch_run(pkg, lbm, [lbm])
        _same(alone[:, 0], sums[:, k])
        assert np.array_equal(s1[:, 0], steps[:, k])
        lbm.close()
    five = _batch(pkg, _batch_params(5))                   # the same replicas inside a batch of 5
    (s5, wide), _ = _batch_run(pkg, five, five.replicas)
    _same(wide[:, :3], sums)
    assert np.array_equal(s5[:, :3], steps)
    five.close()


# ---- 4. the fixture of the CPU oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_record_equals_the_oracle_fixture(pkg, schedule):
    """A 16^3 mixture at kBT = 1e-5 over 40 steps against tests/golden/moment_mixture.npz (make_golden_moment.py): the twin
    applied to the CPU oracle's populations.  The equipartition ratios of the last 20 samples are printed, not asserted."""
    import make_golden_moment as mg
    golden = np.load(GOLDEN)
    lbm = _mixture(pkg, mg.SHAPE, schedule=schedule)
    assert lbm.resolved_schedule() == schedule
    tr = lbm.moment_trace(every=1, capacity=mg.SAMPLES)
    lbm.LBM_timestep(mg.SAMPLES)
    steps, sums = tr.read()
    assert np.array_equal(steps[:, 0], golden["steps"]) and golden["sums"].shape == (mg.SAMPLES, 95)
    _same(sums[:, 0], golden["sums"])
    print(mg.report(golden["sums"], mg.SHAPE[0] * mg.SHAPE[1] * mg.SHAPE[2], pkg.analysis.moment_names()))
    lbm.close()


# ---- 5. lifecycle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_sample_reset_windows_overflow_and_detach(pkg, owner):
    o = _mixture(pkg, BATCH_BOX) if owner == "lone" else _batch(pkg, _batch_params())
    first = o if owner == "lone" else o.replicas[0]
    nrep = 1 if owner == "lone" else 3
    tr = o.moment_trace(every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="moment trace full"):
        o.LBM_timestep(8)
    assert first.steps_done == 0 and tr.count == 0         # refused whole: nothing stepped, nothing recorded
    tr.sample(); tr.sample()                               # twice on the same state
    steps, sums = tr.read()
    assert tr.count == 2 and steps[:, 0].tolist() == [0, 0] and np.array_equal(sums[0], sums[1]) and sums.shape == (2, nrep, 95)
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape == (0, nrep, 95)
    o.LBM_timestep(2)                                      # sample 0 after step 2
    tr.sample()                                            # by hand on the same state: the every-count does not move
    o.LBM_timestep(2)
    assert tr.count == 3 and first.steps_done == 4
    fsteps, full = tr.read()
    assert fsteps[:, 0].tolist() == [2, 2, 4] and np.array_equal(full[0], full[1]) and not np.array_equal(full[1], full[2])
    _same(full[2, 0], _twin(pkg, first))
    with pytest.raises(pkg.BflbmError, match="moment trace full"):
        o.LBM_timestep(2)
    with pytest.raises(pkg.BflbmError, match="moment trace full"):
        tr.sample()
    assert first.steps_done == 4 and tr.count == 3
    wsteps, window = tr.read(first=1, count=2)             # a window of the record
    assert np.array_equal(window, full[1:]) and np.array_equal(wsteps, fsteps[1:])
    assert tr.read(first=3)[1].shape == (0, nrep, 95)
    with pytest.raises(pkg.BflbmError, match="bflbm_moment_read"):
        tr.read(first=2, count=2)
    geo = tr.geometry()
    o.close()                                              # the owner goes first: the trace stays readable with the same bits
    assert tr._h is not None and tr.geometry() == geo
    assert np.array_equal(tr.read()[1], full) and np.array_equal(tr.read()[0], fsteps)
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (10, 6, 13)
    lbm, batch = _mixture(pkg, n), pkg.BatchLBM(n, params=_batch_params())
    for v in batch.replicas:
        v.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_moment_create.*replica of a batch.*use bflbm_batch_moment_create"):
        batch.replicas[0].moment_trace()
    for owner, call in ((lbm, "bflbm_moment_create"), (batch, "bflbm_batch_moment_create")):
        nrep = 3 if owner is batch else 1
        for pattern, kw in (("every must be >= 1", dict(every=0)), ("capacity must be >= 1", dict(capacity=0)),
                            ("capacity must be >= 1", dict(capacity=-3)), ("exceeds 1 TB", dict(capacity=(1 << 37) // (95 * nrep) + 1))):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                owner.moment_trace(**kw)
            assert call in str(e.value), (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
    tr = lbm.moment_trace(capacity=2)
    for bad in (lambda: tr.sums(2), lambda: tr.squares("h")):
        with pytest.raises(ValueError):
            bad()
    tr.close()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_moment_create inside an open step"):
        lbm.moment_trace()
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.moment_trace(capacity=2)
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
    with pytest.raises(pkg.BflbmError, match=r"bflbm_moment_create.*nranks > 1"):
        slab.moment_trace()
    slab.close()


# ---- a recorder changes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["fused", "two_pass"])
def test_a_moment_trace_changes_nothing(pkg, schedule):
    """The populations, the step counter and the noise index (through the noise it draws) of the owner equal those of a run
    without the trace: nothing of the owner is written, not even its scratch state buffer."""
    n = (12, 10, 14)
    a, b = _mixture(pkg, n, schedule), _mixture(pkg, n, schedule)
    tr = a.moment_trace(every=1, capacity=14)              # 13 steps and one sample by hand
    other = a.profile_trace(["rho", "phi"], every=1, capacity=13)         # a recorder that does observe, before and after
    a.LBM_timestep(12); b.LBM_timestep(12)
    assert tr.count == 12 and other.count == 12
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    assert a.steps_done == b.steps_done == 12
    for u, v in zip(a.thermal_noise(), b.thermal_noise()):
        assert np.array_equal(u, v) and np.abs(u).max() > 0
    tr.sample()                                            # by hand: no counter moves
    assert a.steps_done == 12
    a.LBM_timestep(1); b.LBM_timestep(1)                   # the step after the last sample
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    assert np.array_equal(a.LBM_hydrovars(), b.LBM_hydrovars())
    a.close(); b.close()


def test_no_ring_form(pkg):
    assert not hasattr(pkg.RingLBM, "moment_trace")
