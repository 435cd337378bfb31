"""GPU: replica batches (BatchLBM, bflbm_batch_*).  Every replica of a batch must compute, bit for bit, what a lone
BinaryLBM with the same parameters, state, step counter and explicitly forced schedule computes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = np.array([1 / 3] + [1 / 18] * 6 + [1 / 36] * 12)

# replicas differ in alpha0, kappa, rho_hi and tau; inits: droplets of different radii, stripe, mixture, random upload
PARAMS = [dict(alpha0=1.5, kappa=0.1, rho_hi=3.0),
          dict(alpha0=1.7, kappa=1.0, rho_hi=3.0, tau_f=0.7, tau_g=0.7),
          dict(alpha0=2.0, kappa=3.0, rho_hi=2.0),
          dict(alpha0=1.0, kappa=4.0, rho_hi=1.0, tau_f=0.6, tau_g=0.8),
          dict(alpha0=1.2, kappa=2.0, rho_hi=1.5, tau_f=0.55, tau_g=0.55)]
INITS = [("droplet", 0.2), ("droplet", 0.3), ("stripe", 0.5), ("mixture", None), ("random", 7)]


def _random_state(n, seed):
    rng = np.random.default_rng(seed)
    shp = (n[2], n[1], n[0])
    f = W[:, None, None, None] * (0.9 + 0.2 * rng.random((19,) + shp))
    g = W[:, None, None, None] * (0.4 + 0.2 * rng.random((19,) + shp))
    return np.ascontiguousarray(f), np.ascontiguousarray(g)


def _init(lat, n, init):
    kind, arg = init
    if kind == "droplet":
        lat.LBM_init_droplet(arg)
    elif kind == "stripe":
        lat.LBM_init_stripe(arg)
    elif kind == "mixture":
        lat.LBM_init_mixture()
    else:
        lat.LBM_init(*_random_state(n, arg))


def _state(lat):
    f, g = lat.populations()
    return f, g, lat.LBM_hydrovars(), lat.LBM_hydrovars_density()


def _assert_same(a, b, what):
    for x, y, name in zip(_state(a), _state(b), ("f", "g", "hydrovs", "hydrovsbar")):
        assert np.array_equal(x, y), f"{what}: {name} differs, max |d| = {np.nanmax(np.abs(x - y)):.3g}"


def _lones(pkg, n, params, inits, schedule):
    out = []
    for p, init in zip(params, inits):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
        _init(lone, n, init)
        out.append(lone)
    return out


@pytest.mark.parametrize("n,nrep,schedule", [
    ((32, 32, 32), 5, "two_pass"),
    ((64, 64, 64), 3, "fused"),
    ((8, 256, 64), 4, "two_pass"),
    ((8, 256, 64), 4, "fused"),
    ((40, 24, 20), 4, "two_pass"),
    ((40, 24, 20), 4, "fused"),
])
def test_batch_parity_with_lone_lattices(pkg, n, nrep, schedule):
    params, inits = PARAMS[:nrep], INITS[:nrep]
    with pkg.BatchLBM(n, params=params, schedule=schedule) as b:
        assert b.resolved_schedule() == schedule
        for rep, init in zip(b.replicas, inits):
            _init(rep, n, init)
        lones = _lones(pkg, n, params, inits, schedule)
        done = 0
        for upto in (1, 7, 50):
            b.LBM_timestep(upto - done)
            for lone in lones:
                lone.LBM_timestep(upto - done)
            done = upto
            for r, (rep, lone) in enumerate(zip(b.replicas, lones)):
                assert rep.steps_done == lone.steps_done == upto
                _assert_same(rep, lone, f"{n} replica {r} after {upto} steps")
        f, g = b.populations()
        assert f.shape == (nrep, 19, n[2], n[1], n[0])
        assert np.array_equal(f[1], lones[1].populations()[0])
        assert b.LBM_hydrovars().shape == (nrep, 22, n[2], n[1], n[0])
        assert np.array_equal(b.LBM_hydrovars_density()[2], lones[2].LBM_hydrovars_density())
        for lone in lones:
            lone.close()


def test_batch_replica_matches_the_oracle(pkg, ob):
    n = (32, 32, 32)
    with pkg.BatchLBM(n, params=PARAMS[:3], schedule="two_pass") as b:
        for rep, init in zip(b.replicas, INITS[:3]):
            _init(rep, n, init)
        ref = ob.OracleLattice(*n, params=ob.default_params(**PARAMS[1]))
        ref.init_droplet(INITS[1][1])
        for step in range(3):
            b.LBM_timestep(1)
            ref.timestep()
            f, g = b.replicas[1].populations()
            assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g), step
            assert np.array_equal(b.replicas[1].LBM_hydrovars(), ref.h), step


def test_batch_schedules_give_identical_doubles(pkg):
    n = (40, 24, 20)
    out = []
    for plan in (["two_pass"] * 2, ["fused"] * 2, ["two_pass", "fused"]):
        with pkg.BatchLBM(n, params=PARAMS[:4]) as b:
            for rep, init in zip(b.replicas, INITS[:4]):
                _init(rep, n, init)
            for sched in plan:                                             # the same batch switches schedule mid-run
                b.set_schedule(sched)
                b.LBM_timestep(4)
            out.append(b.populations())
    for f, g in out[1:]:
        assert np.array_equal(f, out[0][0]) and np.array_equal(g, out[0][1])


NOISY = [dict(PARAMS[0], kBT=1e-5), dict(PARAMS[1], kBT=3e-5), dict(PARAMS[2], kBT=5e-6)]


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_batch_noise_matches_lone_runs(pkg, schedule):
    n = (32, 32, 32)
    seeds = [11, 12345, 2 ** 40 + 3]
    params = [dict(p, seed=s) for p, s in zip(NOISY, seeds)]
    with pkg.BatchLBM(n, params=params, schedule=schedule) as b:
        if schedule == "two_pass":
            b.set_schedule("auto")
            assert b.resolved_schedule() == "two_pass"                    # auto with noise
        for rep, init in zip(b.replicas, INITS[:3]):
            _init(rep, n, init)
        lones = _lones(pkg, n, params, INITS[:3], schedule)
        b.LBM_timestep(9)
        for lone in lones:
            lone.LBM_timestep(9)
        for r, (rep, lone) in enumerate(zip(b.replicas, lones)):
            _assert_same(rep, lone, f"noisy replica {r}")
            fa, ga = rep.thermal_noise()
            fb, gb = lone.thermal_noise()
            assert np.array_equal(fa, fb) and np.array_equal(ga, gb)
            lone.close()


def test_batch_seeds_and_step_counter(pkg):
    n = (32, 32, 32)
    base = dict(alpha0=1.5, kappa=0.1, rho_hi=3.0, kBT=1e-5, seed=77)
    with pkg.BatchLBM(n, params=base, replicas=4, seeds=[77, 77, 78, 77]) as b:
        assert [p.seed for p in b.params] == [77, 77, 78, 77]
        for rep in b.replicas:
            rep.LBM_init_droplet(0.25)
        b.replicas[3].set_steps_done(1000)                                # shifts only replica 3's noise stream
        b.LBM_timestep(5)
        f, g = b.populations()
        assert np.array_equal(f[0], f[1]) and np.array_equal(g[0], g[1])  # same seed, same state, same counter
        assert not np.array_equal(f[0], f[2])                             # another seed
        assert not np.array_equal(f[0], f[3])                             # another counter
        assert [rep.steps_done for rep in b.replicas] == [5, 5, 5, 1005]
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**base), schedule="two_pass")
        lone.LBM_init_droplet(0.25)
        lone.set_steps_done(1000)
        lone.LBM_timestep(5)
        _assert_same(b.replicas[3], lone, "replica with a shifted step counter")
        lone.close()
    with pkg.BatchLBM(n, params=dict(base, seed=100), replicas=3) as b:   # one dict: seed + r
        assert [p.seed for p in b.params] == [100, 101, 102]


def test_batch_replicas_are_independent(pkg):
    n = (32, 32, 32)
    params, inits = PARAMS[:4], INITS[:4]
    with pkg.BatchLBM(n, params=params, schedule="two_pass") as b:
        for rep, init in zip(b.replicas, inits):
            _init(rep, n, init)
        lones = _lones(pkg, n, params, inits, "two_pass")
        mass0 = [rep.mass() for rep in b.replicas]
        b.LBM_timestep(5)
        for lone in lones:
            lone.LBM_timestep(5)
        # mid-run: re-initialise replica 0, re-upload replica 2, new parameters for replica 3
        b.replicas[0].LBM_init_droplet(0.35)
        lones[0].LBM_init_droplet(0.35)
        f0, g0 = _random_state(n, 99)
        b.replicas[2].LBM_init(f0, g0)
        lones[2].LBM_init(f0, g0)
        b.replicas[3].set_params(alpha0=1.3)
        lones[3].set_params(alpha0=1.3)
        b.LBM_timestep(6)
        for lone in lones:
            lone.LBM_timestep(6)
        for r, (rep, lone) in enumerate(zip(b.replicas, lones)):
            _assert_same(rep, lone, f"replica {r} after the mid-run changes")
        m1 = b.replicas[1].mass()
        np.testing.assert_allclose(m1, mass0[1], rtol=1e-12)              # untouched replica: mass conserved
        for r in (1, 3):
            np.testing.assert_allclose(b.replicas[r].mass(), mass0[r], rtol=1e-12)
        for lone in lones:
            lone.close()


def test_batch_records_follow_a_reinit_and_an_upload_that_keeps_the_counter(pkg):
    """A replica's device record is rewritten because a call marked it stale, not because its step counter or buffer no
    longer follow from the batch steps: right after the step that wrote the records, re-initialise one replica and upload
    into another with commit_upload(False) (same counter, same buffer).  With noise, the counter is the noise index."""
    n = (32, 32, 32)
    params, inits = [dict(p, kBT=1e-5) for p in PARAMS[:3]], INITS[:3]
    with pkg.BatchLBM(n, params=params, schedule="two_pass") as b:
        for rep, init in zip(b.replicas, inits):
            _init(rep, n, init)
        lones = _lones(pkg, n, params, inits, "two_pass")
        b.LBM_timestep(1)
        for lone in lones:
            lone.LBM_timestep(1)
        f1, g1 = _random_state(n, 5)
        for lat in (b.replicas[0], lones[0]):
            lat.LBM_init_droplet(0.35)
        for lat in (b.replicas[1], lones[1]):
            lat.upload(f1, g1)
            lat.commit_upload(False)
        b.LBM_timestep(4)
        for lone in lones:
            lone.LBM_timestep(4)
        assert [rep.steps_done for rep in b.replicas] == [lone.steps_done for lone in lones] == [4, 5, 5]
        for r, (rep, lone) in enumerate(zip(b.replicas, lones)):
            _assert_same(rep, lone, f"replica {r} after a re-init / an upload right after the records were written")
        for lone in lones:
            lone.close()


def test_batch_refusals(pkg):
    n = (32, 32, 32)
    lib = pkg._lib.load()
    with pytest.raises(pkg.BflbmError, match=r"replicas 0, 2 have kBT == 0 and replicas 1 kBT != 0"):
        with pkg.BatchLBM(n, params=[PARAMS[0], dict(PARAMS[1], kBT=1e-5), PARAMS[2]]) as b:
            for rep in b.replicas:
                rep.LBM_init_droplet(0.25)
            b.LBM_timestep(1)
    params, inits = PARAMS[:3], INITS[:3]
    with pkg.BatchLBM(n, params=params, schedule="two_pass") as b:
        for rep, init in zip(b.replicas, inits):
            _init(rep, n, init)
        lones = _lones(pkg, n, params, inits, "two_pass")
        with pytest.raises(pkg.BflbmError, match="schedule 3"):
            b.set_schedule("handover")
        # mixed noise, refused before any launch: nothing advanced
        b.replicas[1].set_params(kBT=1e-5)
        with pytest.raises(pkg.BflbmError, match=r"replicas 0, 2 have kBT == 0 and replicas 1"):
            b.LBM_timestep(1)
        assert [rep.steps_done for rep in b.replicas] == [0, 0, 0]
        b.replicas[1].set_params(kBT=0.0)
        h = b.replicas[0]._h
        dev = ctypes.c_void_p(1)                                         # never dereferenced: the call is refused first
        arr = np.zeros((19, n[2], n[1], n[0]))
        fab = pkg.make_fab((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1))
        ptr = arr.ctypes.data_as(ctypes.c_void_p)
        planes = (ctypes.c_void_p * 64)()
        nb, cnt, sz = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        calls = {
            "bflbm_destroy": (lambda: lib.bflbm_destroy(h), "bflbm_batch_destroy"),
            "bflbm_step": (lambda: lib.bflbm_step(h, 1), "bflbm_batch_step"),
            "bflbm_step_boundary": (lambda: lib.bflbm_step_boundary(h), "bflbm_batch_step"),
            "bflbm_step_interior": (lambda: lib.bflbm_step_interior(h), "bflbm_batch_step"),
            "bflbm_step_finish": (lambda: lib.bflbm_step_finish(h), "bflbm_batch_step"),
            "bflbm_set_schedule": (lambda: lib.bflbm_set_schedule(h, 0), "bflbm_batch_set_schedule"),
            "bflbm_set_stream": (lambda: lib.bflbm_set_stream(h, None, 1), "bflbm_batch_sync"),
            "bflbm_tune_placement": (lambda: lib.bflbm_tune_placement(h, 2, None, None), "bflbm_batch_create"),
            "bflbm_inject_noise": (lambda: lib.bflbm_inject_noise(h, ptr, ptr, ctypes.byref(fab)), "bflbm_batch_step"),
            "bflbm_set_ref_state": (lambda: lib.bflbm_set_ref_state(h, ptr, ptr, ptr, ctypes.byref(fab)), "bflbm_batch_step"),
            "bflbm_enable_ref_state": (lambda: lib.bflbm_enable_ref_state(h, 0, None), "bflbm_batch_step"),
            "bflbm_halo_bytes": (lambda: lib.bflbm_halo_bytes(h, 0, ctypes.byref(sz)), "bflbm_batch_step"),
            "bflbm_halo_pack": (lambda: lib.bflbm_halo_pack(h, 0, 0, dev), "bflbm_batch_step"),
            "bflbm_halo_unpack": (lambda: lib.bflbm_halo_unpack(h, 0, 0, dev), "bflbm_batch_step"),
            "bflbm_halo_planes": (lambda: lib.bflbm_halo_planes(h, 0, 0, 1, planes, ctypes.byref(nb), ctypes.byref(cnt)), "bflbm_batch_step"),
        }
        for name, (call, instead) in calls.items():
            assert call() != 0, f"{name} accepted on a replica view"
            msg = lib.bflbm_last_error().decode()
            assert msg.startswith(name) and instead in msg and "replica of a batch" in msg, msg
        assert [rep.steps_done for rep in b.replicas] == [0, 0, 0]
        # the batch still steps and matches its lone runs
        b.LBM_timestep(7)
        for lone in lones:
            lone.LBM_timestep(7)
        for r, (rep, lone) in enumerate(zip(b.replicas, lones)):
            _assert_same(rep, lone, f"replica {r} after the refusals")
            lone.close()
