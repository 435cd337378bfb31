"""GPU: profile traces (ProfileTrace, bflbm_profile_*): the sums of chosen hydrodynamic variables and of products of them
over every lattice plane normal to one axis, recorded on the device.

The definition and the order of the sums are in include/bflbm.h ("Profile traces"); tests/profile_sums.py writes that
order out site by site (emulate), and tests/test_profile_abi.py holds the numpy twin to it and to the exact sums.  Here
the device record is compared with the emulation of the downloaded fields bit for bit: lone lattices, replicas of a
batch, rings of z-slabs.  The physics pin carries the oracle's figures in its docstring."""
import ctypes
import os

import numpy as np
import pytest

import profile_sums as ps
from test_gpu_notebook_surface_tension import GAMMA_15, GAMMA_17

pytestmark = pytest.mark.gpu

HYD = ["rho", "afz", "agx", "ubx"]                         # of hydrovs; NV = 4
HYD_PAIRS = [("rho", "rho"), ("afz", "agx"), ("ubx", "afz")]
BAR = ["phi", "rho", "ufx"]                                # of hydrovsbar, not in ascending order; NV = 3
BAR_PAIRS = [("phi", "rho"), ("ufx", "ufx")]
AXES = ["x", "y", "z"]


def _start(o, n):
    """A droplet where the box holds one, a stripe in the thin boxes; kBT = 1e-5 leaves no plane uniform."""
    if min(n) >= 5:
        o.LBM_init_droplet(0.3)
    else:
        o.LBM_init_stripe(0.5)


def _lone(pkg, n, schedule=None, **params):
    p = dict(kBT=1e-5, alpha0=2.5, seed=7)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    _start(lbm, n)
    return lbm


def _params():
    return [dict(alpha0=a, kappa=k, tau_f=t, tau_g=t, kBT=kbt, seed=s)
            for a, k, t, kbt, s in zip((2.5, 1.5, 2.0), (4.0, 0.1, 2.0), (0.5, 0.8, 1.0), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


def _batch(pkg, n, schedule=None):
    """Three replicas that differ in parameters, seed and step counter."""
    batch = pkg.BatchLBM(n, params=_params(), schedule=schedule)
    for v in batch.replicas:
        _start(v, n)
    batch.replicas[1].set_steps_done(1000)
    return batch


def _slots(names, pairs):
    return [(names.index(a), names.index(b)) for a, b in pairs]


def _index(pkg, names, bar):
    all_names = pkg.plotfile.variable_names(9 if bar else 22)
    return [all_names.index(v) for v in names]


def _traces(o, **kw):
    """{(source, axis): trace} of the six kinds the definition tests attach."""
    out = {}
    for axis in AXES:
        out[("hydrovs", axis)] = o.profile_trace(HYD, HYD_PAIRS, axis=axis, **kw)
        out[("hydrovsbar", axis)] = o.profile_trace(BAR, BAR_PAIRS, axis=axis, source="hydrovsbar", **kw)
    return out


def _want(pkg, lattice, n):
    """{(source, axis): emulate of the lattice's downloaded fields}."""
    hyd = lattice.LBM_hydrovars()[_index(pkg, HYD, False)]
    bar = lattice.LBM_hydrovars_density()[_index(pkg, BAR, True)]
    out = {}
    for axis in AXES:
        out[("hydrovs", axis)] = ps.emulate(hyd, _slots(HYD, HYD_PAIRS), axis)
        out[("hydrovsbar", axis)] = ps.emulate(bar, _slots(BAR, BAR_PAIRS), axis)
    return out


# ---- 1. against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.BOXES)
def test_lone_record_equals_the_emulation(pkg, n):
    lbm = _lone(pkg, n)
    lbm.LBM_timestep(3)
    traces = _traces(lbm, capacity=1)
    for (source, axis), tr in traces.items():
        nq = (len(HYD) + len(HYD_PAIRS)) if source == "hydrovs" else (len(BAR) + len(BAR_PAIRS))
        assert tr.geometry() == ps.geometry(n, nq, axis), (source, axis)
        tr.sample()
    want = _want(pkg, lbm, n)
    for key, tr in traces.items():
        sums, steps = tr.read()
        assert sums.shape == (1, 1) + want[key].shape and steps.tolist() == [[3]] and steps.dtype == np.int64
        assert np.array_equal(sums[0, 0], want[key]), (n, key, np.abs(sums[0, 0] - want[key]).max())
        assert np.ptp(sums[0, 0, 0]) > 0                   # no uniform profile
        nsites = n[0] * n[1] * n[2] // n[ps.AXES[key[1]]]
        assert np.array_equal(tr.means()[0, 0], sums[0, 0] / float(nsites))
    # the twin on the device's fields
    hyd = lbm.LBM_hydrovars()[_index(pkg, HYD, False)]
    assert np.array_equal(traces[("hydrovs", "z")].read()[0][0, 0], pkg.analysis.plane_profiles(hyd, _slots(HYD, HYD_PAIRS), "z"))
    assert traces[("hydrovs", "y")].names == HYD and traces[("hydrovsbar", "x")].names == BAR
    lbm.close()


@pytest.mark.parametrize("n", ps.BOXES)
def test_batch_record_equals_the_emulation_and_the_lattice_run_alone(pkg, n):
    batch = _batch(pkg, n)
    batch.LBM_timestep(3)
    traces = _traces(batch, capacity=1)
    for tr in traces.values():
        tr.sample()
    got = {key: tr.read() for key, tr in traces.items()}
    for r, v in enumerate(batch.replicas):
        want = _want(pkg, v, n)
        for key, (sums, steps) in got.items():
            assert steps.tolist() == [[3, 1003, 3]] and sums.shape[:2] == (1, 3)
            assert np.array_equal(sums[0, r], want[key]), (n, key, r)
    batch.close()
    for r, p in enumerate(_params()):
        lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p))
        _start(lbm, n)
        if r == 1:
            lbm.set_steps_done(1000)
        lbm.LBM_timestep(3)
        alone = _traces(lbm, capacity=1)
        for key, tr in alone.items():
            tr.sample()
            sums, steps = tr.read()
            assert steps[0, 0] == got[key][1][0, r] and np.array_equal(sums[0, 0], got[key][0][0, r]), (n, key, r)
        lbm.close()


# ---- 2. automatic sampling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n = (9, 7, 5)
    o = _lone(pkg, n) if owner == "lone" else _batch(pkg, n)
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: max(v.steps_done for v in o.replicas) - 1000)
    other = o.trace(every=1, capacity=16)
    tr = o.profile_trace(["rho", "phi"], [("rho", "phi")], axis="z", every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="profile trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    assert tr.count == 1 and tr.read()[1][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    sums, steps = tr.read()
    with pytest.raises(pkg.BflbmError, match="profile trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="profile trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    sums2, steps2 = tr.read()
    assert np.array_equal(sums, sums2) and np.array_equal(steps, steps2)
    assert (steps[:, 0] - steps[0, 0]).tolist() == [0, 1, 2] and steps[0, 0] == 2
    assert not np.array_equal(sums[0], sums[1]) and not np.array_equal(sums[1], sums[2])
    w_sums, w_steps = tr.read(first=1, count=2)                           # a window of the record
    assert np.array_equal(w_sums, sums[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[0].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[1][0, 0] == 7
    # the owner goes first: the trace stays readable with the same bits, refuses a sample, closes twice
    sums, steps = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    sums2, steps2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(sums, sums2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


# ---- 3. independence of what else is attached ------------------------------------------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders(pkg):
    n = (13, 10, 6)
    modes = np.array([(1, 0, 0), (0, 1, 1)])
    records = []
    for order in ("alone", "first", "last"):
        lbm = _lone(pkg, n, schedule="fused")
        mt = fs = None
        if order == "last":
            fs = lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1)
            mt = lbm.mode_trace(["rho", "ubx"], modes, every=1, capacity=8)
        tr = lbm.profile_trace(HYD, HYD_PAIRS, axis="y", every=2, capacity=3)
        if order == "first":
            mt = lbm.mode_trace(["rho", "ubx"], modes, every=1, capacity=8)
            fs = lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1)
        lbm.LBM_timestep(6)
        assert order == "alone" or (mt.count == 6 and fs.count == 6)
        records.append(tr.read() + ((mt.read()[1], fs.cov(0)) if mt else ()))
        lbm.close()
    s0, t0 = records[0]
    assert t0[:, 0].tolist() == [2, 4, 6] and not np.array_equal(s0[0], s0[2])
    for rec in records[1:]:
        assert np.array_equal(rec[0], s0) and np.array_equal(rec[1], t0)
    # nor do the others' records depend on where the profile trace stands
    assert np.array_equal(records[1][2], records[2][2]) and np.array_equal(records[1][3], records[2][3])


# ---- 4. rings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES)
def test_ring_record_equals_the_lone_record(pkg, axis):
    n = (16, 8, 12)
    par = dict(alpha0=2.5, kBT=1e-5, seed=7)
    records = {}
    for nslabs in (0, 1, 2, 3):                            # 0: the lone lattice
        if nslabs == 0:
            o = pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule="fused")
        else:
            o = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**par), schedule="fused")
        o.LBM_init_droplet(0.25)
        hyd = o.profile_trace(HYD, HYD_PAIRS, axis=axis, every=2, capacity=4)
        bar = o.profile_trace(BAR, BAR_PAIRS, axis=axis, source="hydrovsbar", every=3, capacity=2)
        hyd.sample()
        o.LBM_timestep(6)
        records[nslabs] = hyd.read() + bar.read()
        assert hyd.geometry() == ps.geometry(n, 7, axis)
        if nslabs in (2, 3):                               # the last sample against the gathered fields
            want = ps.emulate(o.LBM_hydrovars()[_index(pkg, HYD, False)], _slots(HYD, HYD_PAIRS), axis)
            assert np.array_equal(records[nslabs][0][-1, 0], want), (nslabs, axis)
        # which creation call served the owner: a ring of one slab gets the lone recorder
        with pytest.raises(pkg.BflbmError) as e:
            o.profile_trace(["rho"], axis=axis, every=0)
        assert ("bflbm_ring_profile_create" if nslabs > 1 else "bflbm_profile_create") in str(e.value)
        o.close()
    lone = records[0]
    assert lone[1][:, 0].tolist() == [0, 2, 4, 6] and lone[3][:, 0].tolist() == [3, 6] and np.ptp(lone[0][1, 0, 1]) > 0
    for nslabs in (1, 2, 3):
        for a, b in zip(records[nslabs], lone):
            assert np.array_equal(a, b), (nslabs, axis)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm, batch = _lone(pkg, n), _batch(pkg, n)
    ring = pkg.RingLBM(*n, nslabs=2, devices=(0,), params=pkg.default_params(kBT=1e-5))
    ring.LBM_init_droplet(0.25)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_profile_create.*replica of a batch.*use bflbm_batch_profile_create"):
        batch.replicas[0].profile_trace(["rho"])
    for owner, call in ((lbm, "bflbm_profile_create"), (batch, "bflbm_batch_profile_create"), (ring, "bflbm_ring_profile_create")):
        nrep = 3 if owner is batch else 1
        for pattern, variables, pairs, kw in (("variable index 22 outside hydrovs", [0, 22], [], {}),
                                              ("variable index -1 outside hydrovs", [-1], [], {}),
                                              ("variable index 9 outside hydrovsbar", [9], [], dict(source="hydrovsbar")),
                                              ("variable index 3 given twice", [3, 1, 3], [], {}),
                                              ("1..8 variables", list(range(9)), [], {}),
                                              ("1..8 variables", [], [], {}),
                                              ("0..16 pairs", [0], [(0, 0)] * 17, {}),
                                              ("pair 1: slot 2 outside the 2 variables", [0, 1], [(0, 1), (2, 0)], {}),
                                              ("pair 0: slot -1 outside the 1 variables", [0], [(0, -1)], {}),
                                              ("source must be 0", [0], [], dict(source=2)),
                                              ("axis must be 0", [0], [], dict(axis=3)),
                                              ("every must be >= 1", [0], [], dict(every=0)),
                                              ("capacity must be >= 1", [0], [], dict(capacity=0)),
                                              ("exceeds 1 TB", [0], [], dict(capacity=(1 << 37) // (8 * nrep) + 1))):
            direct = {k: kw.pop(k) for k in ("source", "axis") if k in kw and not isinstance(kw[k], str)}
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                if direct:                                 # past the wrapper's own checks: through the ABI
                    h = ctypes.c_void_p()
                    va = (ctypes.c_int * 1)(0)
                    pkg._lib.check(getattr(pkg._lib.load(), call)(owner._h, direct.get("source", 0), direct.get("axis", 2), 1, va, 0, None, None,
                                                                  1, 4, ctypes.byref(h)))
                else:
                    owner.profile_trace(variables, pairs, **kw)
            assert call in str(e.value), (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        full = owner.profile_trace(list(range(8)), [(k % 8, (3 * k) % 8) for k in range(16)], capacity=1)      # the limits themselves
        full.sample()
        assert full.geometry()[0] == 24 and np.isfinite(full.read()[0]).all()
        full.close()
    for bad in (lambda: lbm.profile_trace(["no_such_variable"]), lambda: lbm.profile_trace(["rho"], [("phi", "rho")]),
                lambda: lbm.profile_trace(["rho"], axis="w"), lambda: lbm.profile_trace(["rho"], source="noise")):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_profile_create inside an open step"):
        lbm.profile_trace(["rho"])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.profile_trace(["rho"], capacity=2)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[1][:, 0].tolist() == [1, 2]       # the split step samples in its finish
    lbm.close(); batch.close(); ring.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_profile_create.*nranks > 1"):
        slab.profile_trace(["rho"])
    slab.close()


def test_profile_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lone(pkg, (9, 7, 5))
    t = ctypes.c_void_p()
    va, pa, pb = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    check(lib.bflbm_profile_create(lbm._h, 1, 0, 2, va, 1, pa, pb, 1, 4, ctypes.byref(t)))
    lbm.LBM_timestep(3)

    def read(first, count):
        sums, steps = np.empty((count, 1, 3, 9)), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_profile_read(t, first, count, sums.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return sums, steps
    sums0, steps0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3]
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    sums1, steps1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(sums0, sums1)
    assert np.array_equal(read(2, 1)[0][0], sums0[2])      # a window
    assert lib.bflbm_profile_read(t, 2, 2, sums0.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.bflbm_profile_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_profile_destroy(t))


# ---- 6. the mechanical surface tension of a flat stripe ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_stripe.npz")


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("case,alpha0,kappa,laplace", [("a15_k01", 1.5, 0.1, GAMMA_15[2]), ("a17_k10", 1.7, 1.0, GAMMA_17[2])])
def test_stripe_pressure_profile_gives_the_mechanical_surface_tension(pkg, case, alpha0, kappa, laplace, schedule):
    """An 8 x 8 x 64 stripe (frac = 0.5, rho_hi = 3, tau = 1/2, kBT = 0) after 20000 steps: one sample of the pressure
    variables along z equals the CPU oracle's record (tests/golden/profile_stripe.npz, make_golden_profile.py) bit for
    bit, and gamma_mech = 1/2 sum_z (P_N - P_T) against the Laplace-law value of Surface_Tension.ipynb's droplets, which
    is in units of a 32-cell box: gamma_mech / (32 GAMMA[2]) in [0.96, 0.99].  The CPU oracle gives, on this box,
        alpha0 1.5, kappa 0.1:  gamma_mech = 0.33587892397, ratio 0.9733
        alpha0 1.7, kappa 1.0:  gamma_mech = 0.42026974490, ratio 0.9759
    The gap is the truncation of the notebook's continuum tensor, not noise; a wrong sign, a factor 2, a missing
    1 / alpha0 or 1 / interfaces falls far outside the band."""
    golden = {k.replace("__", "/"): v for k, v in np.load(GOLDEN).items()}
    n = tuple(int(v) for v in golden["shape"])
    variables, pairs = pkg.analysis.pressure_profile_inputs()
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(rho_hi=3.0, rho_lo=0.0, tau_f=0.5, tau_g=0.5, kBT=0.0, alpha0=alpha0, kappa=kappa),
                        schedule=schedule)
    lbm.LBM_init_stripe(0.5)
    lbm.LBM_timestep(int(golden["steps"]))
    tr = lbm.profile_trace(variables, pairs, axis="z", capacity=1)
    tr.sample()
    sums, steps = tr.read()
    assert steps.tolist() == [[int(golden["steps"])]] and tr.names == variables
    p_bulk, pnt = pkg.analysis.pressure_profile(tr.means()[0, 0], tr.names, alpha0, lbm.params.cs2, "z")
    gamma = float(pkg.analysis.mechanical_surface_tension(pnt, interfaces=2))
    ratio = gamma / (32.0 * laplace)
    print("%s %s: gamma_mech = %.11f (oracle %.11f), gamma_mech / (32 x %.15g) = %.4f, largest |u_f| = %.3g"
          % (case, schedule, gamma, float(golden["gamma/" + case]), laplace, ratio, np.abs(lbm.LBM_hydrovars()[2:5]).max()))
    assert np.array_equal(sums[0, 0], golden["sums/" + case]), np.abs(sums[0, 0] - golden["sums/" + case]).max()
    assert 0.96 <= ratio <= 0.99, ratio
    lbm.close()
