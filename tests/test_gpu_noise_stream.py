"""GPU: the noise stream the DEVICE generates -- bit for bit the oracle's, then through the distribution and independence
battery of tests/noise_battery.py (tests/test_noise_battery.py runs it on the oracle's fields and shows its teeth).

  lone lattice   64 x 64 x 32 mixture (rho = phi = 1, alpha0 = 0, tau = 1, kBT = 1e-5): thermal_noise() at seed 12345, noise
                 indices 0 and 1 (set_steps_done; the populations stay), and at seed 12346 == ob.thermal_noise; the battery
                 on the device's fields: 6568 tests, the figures of tests/test_noise_battery.py since the levels are equal
  ring           3 slabs of the same box: the lone lattice's field (the site index is global)
  batch          BatchLBM((64, 32, 16), seed=777, replicas=4) at step count 5: each replica == the lone lattice of its seed;
                 the six cross-replica matrices through check: the independence that seed + r promises
  high key word  seeds 12345 and 12345 + 2^32 differ, each == the oracle's
  index edges    a droplet (kBT = 1e-5, alpha0 = 1) on 128 x 8 x 8 under two_pass, fused and handover, and on a 2-slab ring
                 of 128 x 8 x 16 (fused, handover): the step counter set to 2^31 - 1 and to 2^32 - 1, then two steps.  The
                 exact schedules equal the oracle bit for bit in populations and thermal_noise() after each step; handover
                 after its first step, and within 1e-13 after the second (its contract, tests/test_gpu_handover_oracle.py);
                 steps_done reports the unwrapped count.
Nothing here is a measured tolerance: bit equality, the derived thresholds of noise_battery.thresholds, and 1e-13."""
import numpy as np
import pytest

import noise_battery as nb

pytestmark = pytest.mark.gpu

PAR = dict(kBT=1e-5, alpha0=0.0, tau_f=1.0, tau_g=1.0)
BASE = (64, 64, 32)
BATCH = (64, 32, 16)
BATCH_SEEDS, BATCH_INDEX = [777, 778, 779, 780], 5

_device = {}
_oracle = {}
_mixture = {}


@pytest.fixture()
def threads(ob):
    ob.lib().orc_set_threads(16)
    yield
    ob.lib().orc_set_threads(1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _amplitudes(ob):
    return nb.unit_state_amplitudes(ob.lattice_tables()[2], kBT=PAR["kBT"], tau=PAR["tau_f"])


def _oracle_noise(ob, n, seed, index):
    """ob.thermal_noise on the densities of the oracle's own mixture state, once per case."""
    key = (n, seed, index)
    if key not in _oracle:
        mix = _mixture.get(n)
        if mix is None:
            ref = ob.OracleLattice(*n, params=ob.default_params(seed=seed, **PAR))
            ref.init_mixture()
            mix = _mixture[n] = (ref.hbar[0].copy(), ref.hbar[1].copy())
            assert np.abs(mix[0] - 1.0).max() < 4e-15 and np.abs(mix[1] - 1.0).max() < 4e-15
        _oracle[key] = ob.thermal_noise(n, ob.default_params(seed=seed, **PAR), mix[0], mix[1], noise_index=index)
    return _oracle[key]


def _device_noise(pkg, n, seed, indices):
    """thermal_noise() of a lone mixture lattice at each noise index, moved with set_steps_done; once per case."""
    if not all((n, seed, i) in _device for i in indices):
        with pkg.BinaryLBM(*n, params=pkg.default_params(seed=seed, **PAR)) as lbm:
            lbm.LBM_init_mixture()
            f0, g0 = lbm.populations()
            for i in indices:
                lbm.set_steps_done(i)
                assert lbm.steps_done == i
                _device[(n, seed, i)] = lbm.thermal_noise()
            f1, g1 = lbm.populations()
            assert _same(f0, f1) and _same(g0, g1), "set_steps_done changed the state"
    return [_device[(n, seed, i)] for i in indices]


def _assert_oracle_field(ob, got, n, seed, index):
    want = _oracle_noise(ob, n, seed, index)
    assert np.abs(got[0]).max() > 1e-4
    assert _same(got[0], want[0]) and _same(got[1], want[1]), f"{n} seed {seed} index {index}: the device's noise is not the oracle's"


def test_lone_lattice_stream_is_the_oracles_and_passes_the_battery(pkg, ob, threads):
    (d0, d1), (d2,) = _device_noise(pkg, BASE, 12345, [0, 1]), _device_noise(pkg, BASE, 12346, [0])
    for got, seed, index in ((d0, 12345, 0), (d1, 12345, 1), (d2, 12346, 0)):
        _assert_oracle_field(ob, got, BASE, seed, index)
    amp = _amplitudes(ob)
    S, S1, S2 = (nb.levels(fn, gn, amp) for fn, gn in (d0, d1, d2))
    stats = nb.battery(S, BASE, S_next_index=S1, S_other_seed=S2)
    thr = nb.thresholds(stats)
    assert thr["ntests"] == 6568
    nb.check(stats, thr, f"device {BASE} seed 12345 index 0")


def test_ring_stream_is_the_lone_lattices(pkg, ob):
    (lone,) = _device_noise(pkg, BASE, 12345, [0])
    ring = pkg.RingLBM(*BASE, nslabs=3, devices=(0,), params=pkg.default_params(seed=12345, **PAR))
    try:
        assert sorted(s.nzl for s in ring.slabs) == [10, 11, 11]
        ring.LBM_init_mixture()
        fn, gn = ring.thermal_noise()
    finally:
        ring.close()
    assert _same(fn, lone[0]) and _same(gn, lone[1])


def test_batch_replicas_draw_the_streams_of_their_seeds_and_these_are_independent(pkg, ob, threads):
    with pkg.BatchLBM(BATCH, params=dict(PAR, seed=BATCH_SEEDS[0]), replicas=len(BATCH_SEEDS)) as b:
        assert [int(p.seed) for p in b.params] == BATCH_SEEDS
        for rep in b.replicas:
            rep.LBM_init_mixture()
            rep.set_steps_done(BATCH_INDEX)
        assert [rep.steps_done for rep in b.replicas] == [BATCH_INDEX] * len(BATCH_SEEDS)
        fields = [rep.thermal_noise() for rep in b.replicas]
    amp = _amplitudes(ob)
    streams = []
    for seed, (fn, gn) in zip(BATCH_SEEDS, fields):
        (lone,) = _device_noise(pkg, BATCH, seed, [BATCH_INDEX])
        assert _same(fn, lone[0]) and _same(gn, lone[1]), f"replica with seed {seed}"
        _assert_oracle_field(ob, (fn, gn), BATCH, seed, BATCH_INDEX)
        streams.append(nb.levels(fn, gn, amp))
    stats = nb.cross_seed_pairs(streams)
    assert stats["next_seed"]["ntests"] == 6 * 1089
    nb.check(stats, nb.thresholds(stats), f"device batch {BATCH} seeds 777..780 index {BATCH_INDEX}, six pairs")


def test_high_word_of_the_seed_reaches_the_key(pkg, ob, threads):
    (lo,), (hi,) = _device_noise(pkg, BASE, 12345, [0]), _device_noise(pkg, BASE, 12345 + 2 ** 32, [0])
    assert not np.array_equal(lo[0], hi[0]) and not np.array_equal(lo[1], hi[1])
    _assert_oracle_field(ob, lo, BASE, 12345, 0)
    _assert_oracle_field(ob, hi, BASE, 12345 + 2 ** 32, 0)
    amp = _amplitudes(ob)
    stats = dict(next_seed=nb.cross_seed(nb.levels(*lo, amp), nb.levels(*hi, amp)))
    nb.check(stats, nb.thresholds(stats), f"device {BASE} seeds 12345, 12345 + 2^32")


# ---- index edges ------------------------------------------------------------------------------------------------------------
EDGE_PAR = dict(kBT=1e-5, alpha0=1.0)


def _droplet_radius(shape):
    """LBM_init_droplet centres the droplet at z = nx / 2 (LBM_binary.H:725), outside a flat lattice: this radius lets the
    sphere reach 0.03 nx planes into the box (as in tests/test_gpu_handover_oracle.py)."""
    nx, _, nz = shape
    return max(0.2, 0.5 - (nz - 1) / nx + 0.03)


@pytest.mark.parametrize("start", [2 ** 31 - 1, 2 ** 32 - 1], ids=["2^31-1", "2^32-1"])
@pytest.mark.parametrize("shape,nslabs,schedule", [((128, 8, 8), 1, "two_pass"), ((128, 8, 8), 1, "fused"), ((128, 8, 8), 1, "handover"),
                                                   ((128, 8, 16), 2, "fused"), ((128, 8, 16), 2, "handover")],
                         ids=["two_pass", "fused", "handover", "ring2-fused", "ring2-handover"])
def test_noise_index_across_the_edges_of_32_bits(pkg, ob, threads, shape, nslabs, schedule, start):
    r = _droplet_radius(shape)
    ref = ob.OracleLattice(*shape, params=ob.default_params(**EDGE_PAR))
    ref.init_droplet(r)
    ref.steps = start
    ref.refresh()                                                         # the binding passes c_uint32(steps): the same wrap
    p = pkg.default_params(**EDGE_PAR)
    lbm = pkg.BinaryLBM(*shape, params=p, schedule=schedule) if nslabs == 1 else \
        pkg.RingLBM(*shape, nslabs=nslabs, devices=(0,), params=p, schedule=schedule)
    try:
        assert (lbm if nslabs == 1 else lbm.slabs[0]).resolved_schedule() == schedule
        lbm.LBM_init_droplet(r)
        lbm.set_steps_done(start)
        fn, gn = lbm.thermal_noise()
        assert np.abs(fn).max() > 1e-5
        assert _same(fn, ref.fn) and _same(gn, ref.gn), "before the steps"
        for k in (1, 2):
            lbm.LBM_timestep(1)
            ref.timestep()
            assert lbm.steps_done == ref.steps == start + k
            f, g = lbm.populations()
            fn, gn = lbm.thermal_noise()
            assert np.isfinite(ref.f).all() and np.isfinite(ref.g).all()
            if schedule != "handover" or k == 1:
                assert _same(f, ref.f) and _same(g, ref.g), f"populations after step {k}"
                assert _same(fn, ref.fn) and _same(gn, ref.gn), f"noise after step {k}"
            else:
                err = max(np.abs(f - ref.f).max(), np.abs(g - ref.g).max())
                nerr = max(np.abs(fn - ref.fn).max(), np.abs(gn - ref.gn).max())
                print(f"{shape} / {nslabs} handover from {start}: step 2 populations {err:.3e}, noise {nerr:.3e} / 1e-13")
                assert err < 1e-13 and nerr < 1e-13
    finally:
        lbm.close()
