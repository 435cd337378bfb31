"""GPU: the three recorder kinds (moments trace, interface trace, batch structure factor) on one owner, through the one
lifecycle of csrc/bflbm_recorder.h.  No kind reads what another writes, so every recorded double and every label must
be equal bit for bit whether a recorder is alone on its owner or shares it, and whatever the creation order is; all
kinds outlive their owner; a full recorder of either trace kind refuses the step before any launch.
8 x 8 x 8 is the smallest shape that still covers the risks: a ragged 256-site block in stage 1, a window that starts
and ends inside the lattice, and an `every` that skips steps."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (8, 8, 8)
PARAMS = dict(alpha0=1.5, rho_lo=0.1, rho_hi=3.0, kappa=0.1, kBT=1e-5)      # the stripe of tests/test_gpu_iface.py
SEEDS = [21, 22]
LEVEL, WINDOW = 1.55, (1, 7)
NREC = 12


def _names(pkg):
    return pkg.plotfile.variable_names(22)


def _makers(pkg):
    return {"trace": lambda b: b.trace(every=1, capacity=4),
            "rho": lambda b: b.interface_trace(LEVEL, field="rho", window=WINDOW, every=2, capacity=2),
            "phi": lambda b: b.interface_trace(LEVEL, field="phi", window=WINDOW, every=2, capacity=2),
            "sf": lambda b: b.structfact(_names(pkg), every=2)}


def _output(ob):
    if hasattr(ob, "means"):
        return np.array([ob.nsamples]), ob.means()
    return ob.read()


def _run(pkg, kinds):
    """A batch of 2 stripes carrying the recorders `kinds`, created in that order, after 4 steps: what each recorder
    returns, and the populations."""
    batch = pkg.BatchLBM(N, params=PARAMS, replicas=2, seeds=SEEDS)
    for rep in batch.replicas:
        rep.LBM_init_stripe(0.5)
    makers = _makers(pkg)
    obs = {kind: makers[kind](batch) for kind in kinds}
    batch.LBM_timestep(4)
    out = {kind: _output(ob) for kind, ob in obs.items()}
    pops = batch.populations()
    for ob in obs.values():
        ob.close()
    batch.close()
    return out, pops


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


KINDS = ["trace", "rho", "phi", "sf"]


@pytest.fixture(scope="module")
def combined(pkg):
    return _run(pkg, KINDS)


def test_all_kinds_on_one_batch_equal_each_kind_alone(pkg, combined):
    out, pops = combined
    assert out["trace"][0].tolist() == [[1, 1], [2, 2], [3, 3], [4, 4]]
    assert out["rho"][0].tolist() == out["phi"][0].tolist() == [[2, 2], [4, 4]]
    assert out["sf"][0].tolist() == [2]
    assert out["trace"][1].shape == (4, 2, NREC) and out["rho"][1].shape == (2, 2, 2, 8, 8)
    assert out["sf"][1].shape == (2, 22, 8, 8, 8)
    assert np.isfinite(out["rho"][1]).any() and np.isfinite(out["phi"][1]).any()      # the window holds a crossing
    for kind in KINDS:
        alone, pops_alone = _run(pkg, [kind])
        for u, v in zip(alone[kind], out[kind]):
            assert _bits(u, v), kind
        for u, v in zip(pops_alone, pops):
            assert _bits(u, v), kind


def test_creation_order_changes_no_value(pkg, combined):
    out, pops = combined
    reverse, pops_reverse = _run(pkg, KINDS[::-1])
    for kind in KINDS:
        for u, v in zip(reverse[kind], out[kind]):
            assert _bits(u, v), kind
    for u, v in zip(pops_reverse, pops):
        assert _bits(u, v)


# ---- lifetime, through the raw ABI as tests/test_gpu_trace.py::test_trace_outlives_its_owner ------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _store_reader(lib, check, prefix, handle, shape):
    def read():
        n, b = ctypes.c_longlong(), ctypes.c_int()
        check(getattr(lib, prefix + "_count")(handle, ctypes.byref(n), ctypes.byref(b)))
        rec = np.empty((n.value, b.value) + shape)
        steps = np.empty((n.value, b.value), dtype=np.int64)
        check(getattr(lib, prefix + "_read")(handle, 0, n.value, _ptr(rec), _ptr(steps)))
        return steps, rec
    return read


def _outlive(lib, readers, samplers, destroy_owner, destroyers):
    before = [read() for read in readers]
    destroy_owner()
    after = [read() for read in readers]
    for x, y in zip(before, after):
        for u, v in zip(x, y):
            assert _bits(u, v)
    for sample in samplers:
        assert sample() != 0
        assert "destroyed" in lib.bflbm_last_error().decode()
    for destroy in destroyers:
        destroy()
    return before


def _batch_outlived(pkg, lib, check):
    params = (pkg.Params * 2)(*[pkg.default_params(**dict(PARAMS, seed=s)) for s in SEEDS])
    b, t, i, s = (ctypes.c_void_p() for _ in range(4))
    check(lib.bflbm_batch_create(params, 2, (ctypes.c_int * 3)(*N), 0, ctypes.byref(b)))
    for r in range(2):
        c = ctypes.c_void_p()
        check(lib.bflbm_batch_replica(b, r, ctypes.byref(c)))
        check(lib.bflbm_init_stripe(c, 0.5))
    pair_a, pair_b = (ctypes.c_int * 2)(0, 0), (ctypes.c_int * 2)(0, 1)
    check(lib.bflbm_batch_trace_create(b, 1, 8, -np.inf, ctypes.byref(t)))
    check(lib.bflbm_batch_iface_create(b, 0, LEVEL, WINDOW[0], WINDOW[1], 1, 8, ctypes.byref(i)))
    check(lib.bflbm_batch_sf_create(b, 2, pair_a, pair_b, None, 0, 1, ctypes.byref(s)))
    check(lib.bflbm_trace_sample(t))
    check(lib.bflbm_iface_sample(i))
    check(lib.bflbm_batch_sf_accumulate(s, 0))
    check(lib.bflbm_batch_step(b, 2))

    def spectra():
        n = ctypes.c_longlong()
        check(lib.bflbm_batch_sf_nsamples(s, ctypes.byref(n)))
        out = np.empty((3, 2, 2) + N[::-1])                              # [ensemble mean, replica 0, replica 1][Re, Im]
        for k, replica in enumerate((-1, 0, 1)):
            for what in (1, 2):
                check(lib.bflbm_batch_sf_get(s, replica, what, 0, _ptr(out[k, what - 1])))
        return np.array([n.value]), out

    before = _outlive(lib, [_store_reader(lib, check, "bflbm_trace", t, (NREC,)),
                            _store_reader(lib, check, "bflbm_iface", i, (2, N[1], N[0])), spectra],
                      [lambda: lib.bflbm_trace_sample(t), lambda: lib.bflbm_iface_sample(i),
                       lambda: lib.bflbm_batch_sf_accumulate(s, 0)],
                      lambda: check(lib.bflbm_batch_destroy(b)),
                      [lambda: check(lib.bflbm_trace_destroy(t)), lambda: check(lib.bflbm_iface_destroy(i)),
                       lambda: check(lib.bflbm_batch_sf_destroy(s))])
    assert before[0][0].tolist() == before[1][0].tolist() == [[0, 0], [1, 1], [2, 2]]
    assert before[2][0].tolist() == [3] and np.abs(before[2][1]).max() > 0


def _lone_context_outlived(pkg, lib, check):
    p = pkg.default_params(**PARAMS)
    d = pkg.Domain()
    d.n[0], d.n[1], d.n[2] = N
    d.z0, d.z1, d.rank, d.nranks, d.device = 0, N[2], 0, 1, 0
    c, t, i = (ctypes.c_void_p() for _ in range(3))
    check(lib.bflbm_create(ctypes.byref(p), ctypes.byref(d), ctypes.byref(c)))
    check(lib.bflbm_init_stripe(c, 0.5))
    check(lib.bflbm_trace_create(c, 1, 8, -np.inf, ctypes.byref(t)))
    check(lib.bflbm_iface_create(c, 0, LEVEL, WINDOW[0], WINDOW[1], 1, 8, ctypes.byref(i)))
    check(lib.bflbm_trace_sample(t))
    check(lib.bflbm_iface_sample(i))
    check(lib.bflbm_step(c, 2))
    before = _outlive(lib, [_store_reader(lib, check, "bflbm_trace", t, (NREC,)),
                            _store_reader(lib, check, "bflbm_iface", i, (2, N[1], N[0]))],
                      [lambda: lib.bflbm_trace_sample(t), lambda: lib.bflbm_iface_sample(i)],
                      lambda: check(lib.bflbm_destroy(c)),
                      [lambda: check(lib.bflbm_trace_destroy(t)), lambda: check(lib.bflbm_iface_destroy(i))])
    assert before[0][0].tolist() == before[1][0].tolist() == [[0], [1], [2]]


def test_all_kinds_outlive_the_owner(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    _batch_outlived(pkg, lib, check)
    _lone_context_outlived(pkg, lib, check)


# ---- overflow ---------------------------------------------------------------------------------------------------------------
def test_overflow_of_either_kind_refuses_the_step_before_any_launch(pkg):
    lbm = pkg.BinaryLBM(*N, params=pkg.default_params(**PARAMS))
    lbm.LBM_init_stripe(0.5)
    tr = lbm.trace(every=1, capacity=4)
    it = lbm.interface_trace(LEVEL, window=WINDOW, every=1, capacity=2)
    state = lbm.populations()
    with pytest.raises(pkg.BflbmError, match="interface trace full"):
        lbm.LBM_timestep(3)                                              # the trace would hold them, the interface trace not
    assert lbm.steps_done == 0 and tr.count == 0 and it.count == 0
    assert all(_bits(u, v) for u, v in zip(state, lbm.populations()))
    lbm.close()
