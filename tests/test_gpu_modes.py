"""GPU: mode traces (ModeTrace, bflbm_modes_*): the complex Fourier amplitudes of chosen hydrodynamic variables at
chosen wavevectors, recorded on the device.

The definition and the order of the sums are in include/bflbm.h ("Mode traces"); tests/mode_sums.py holds the numpy
emulation of that order, the exact reference and the bound depth_bound(nx, ny, nz) against sum |a|.  The exact tests
compare bits; the physics tests (sign and scale, the Onsager regression, the shear wave) carry the figures of the CPU
oracle in their docstrings."""
import ctypes

import numpy as np
import pytest

import mode_sums as ms
import relaxation_cases as rc

pytestmark = pytest.mark.gpu

BOXES = [(13, 10, 6), (40, 9, 5)]
BAR = ["rho", "phi", "ufx"]                                # of hydrovsbar
HYD = ["rho", "ubx", "uby"]                                # of hydrovs


def _lone(pkg, n, schedule=None, **params):
    p = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_mixture()
    return lbm


def _params():
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


def _batch(pkg, n, schedule=None):
    """Three replicas that differ in parameters, seed and step counter (tests/test_gpu_spectrum.py)."""
    batch = pkg.BatchLBM(n, params=_params(), schedule=schedule)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    return batch


def _index(pkg, names, lb):
    all_names = pkg.plotfile.variable_names(9 if lb else 22)
    return [all_names.index(v) for v in names]


# ---- 1. exact integers -----------------------------------------------------------------------------------------------------
def _quarter_modes(n):
    nx, ny, nz = n
    return np.array([(nx // 2, 0, 0), (nx // 4, ny // 4, nz // 4), (-(nx // 4), ny // 2, nz // 4), (0, 0, 0),
                     (3 * nx // 4, 3 * ny // 4, 3 * nz // 4)])


def _integer_dft(k_zyx, modes):
    """[(re, im)] in Python integers: every phase is a power of -i."""
    nz, ny, nx = k_zyx.shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    out = []
    for mx, my, mz in modes.tolist():
        assert (4 * mx) % nx == 0 and (4 * my) % ny == 0 and (4 * mz) % nz == 0
        q = (4 * mx // nx * x + 4 * my // ny * y + 4 * mz // nz * z) % 4         # E = (-i)^q
        s = [int(k_zyx[q == r].sum()) for r in range(4)]
        out.append((s[0] - s[2], s[3] - s[1]))
    return out


def _integer_state(n, seed):
    nx, ny, nz = n
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 1000, size=(2, nz, ny, nx))
    f0 = np.zeros((19, nz, ny, nx)); g0 = np.zeros((19, nz, ny, nx))
    f0[0] = k[0]; g0[0] = k[1]
    return k, f0, g0


@pytest.mark.parametrize("n", [(16, 12, 8), (20, 12, 8), (4112, 16, 4)])
def test_integer_fields_give_the_integer_dft_exactly(pkg, n):
    modes = _quarter_modes(n)
    k, f0, g0 = _integer_state(n, 7)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0, alpha0=0.0))
    lbm.LBM_init(f0, g0)
    tr = lbm.mode_trace(["rho", "phi"], modes, capacity=1, lb_hydrovars=True)
    assert tr.geometry() == (2, 5, ms.tiles_per_plane(n[0], n[1]), ms.TILE)
    tr.sample()
    steps, amp = tr.read()
    assert amp.shape == (1, 1, 2, 5) and amp.dtype == np.complex128 and steps.tolist() == [[0]]
    for v in range(2):
        want = _integer_dft(k[v], modes)
        got = [(int(a.real), int(a.imag)) for a in amp[0, 0, v]]
        assert amp[0, 0, v].real.tolist() == [float(w[0]) for w in want] and got == want, (n, v, got, want)
    lbm.close()


def test_integer_fields_in_a_batch(pkg):
    n = (20, 12, 8)
    modes = _quarter_modes(n)
    batch = pkg.BatchLBM(n, params=dict(kBT=0.0, alpha0=0.0), replicas=2)
    ks = []
    for r, v in enumerate(batch.replicas):
        k, f0, g0 = _integer_state(n, 20 + r)
        v.LBM_init(f0, g0)
        ks.append(k)
    tr = batch.mode_trace(["phi", "rho"], modes, capacity=1, lb_hydrovars=True)      # not in ascending order
    tr.sample()
    amp = tr.read()[1]
    for r in range(2):
        for v, which in enumerate((1, 0)):
            assert [(int(a.real), int(a.imag)) for a in amp[0, r, v]] == _integer_dft(ks[r][which], modes)
    batch.close()


# ---- 2. against the definition ------------------------------------------------------------------------------------------------
def _check_record(pkg, amp, fields, n, modes, tables, what):
    """amp[nvars, nmodes] against fields[nvars, nz, ny, nx]: inside depth_bound of the longdouble projection with the
    library's tables, and the bits of the emulation."""
    bound = ms.depth_bound(*n)
    worst = 0.0
    for v in range(len(fields)):
        want = ms.longdouble_projection(fields[v], modes, tables)
        worst = max([worst] + [ms.ratio_to_bound(a, w, np.abs(fields[v]).sum(), bound) for a, w in zip(amp[v], want)])
        assert np.array_equal(amp[v], ms.emulate(fields[v], modes, tables)), (what, v)
    print(what, "worst |device - longdouble| / (depth_bound sum |a|) = %.3g" % worst)
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("n", BOXES)
def test_lone_record_against_the_definition(pkg, n, schedule):
    tables = ms.tables_of(pkg._lib.load(), n)
    modes = ms.issue_modes(n)
    lbm = _lone(pkg, n, schedule)
    lbm.LBM_timestep(5)
    hyd = lbm.mode_trace(HYD, modes, capacity=1)
    bar = lbm.mode_trace(_index(pkg, BAR, True), modes, capacity=1, lb_hydrovars=True)
    hyd.sample(); bar.sample()
    _check_record(pkg, hyd.read()[1][0, 0], lbm.LBM_hydrovars()[_index(pkg, HYD, False)], n, modes, tables, (n, schedule, "hydrovs"))
    _check_record(pkg, bar.read()[1][0, 0], lbm.LBM_hydrovars_density()[_index(pkg, BAR, True)], n, modes, tables, (n, schedule, "hydrovsbar"))
    # one variable against the exact sums in Fractions, and the numpy definition to its own rounding
    rho = lbm.LBM_hydrovars_density()[0]
    exact = ms.exact(rho, modes, tables)
    got = bar.read()[1][0, 0, 0]
    assert max(ms.ratio_to_bound(a, w, np.abs(rho).sum(), ms.depth_bound(*n)) for a, w in zip(got, exact)) <= 1.0
    assert np.abs(got - pkg.analysis.fourier_modes(rho, modes)).max() <= 1e-12 * np.abs(rho).sum()
    lbm.close()


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("n", BOXES)
def test_batch_record_against_the_definition(pkg, n, schedule):
    tables = ms.tables_of(pkg._lib.load(), n)
    modes = ms.issue_modes(n)
    batch = _batch(pkg, n, schedule)
    batch.LBM_timestep(5)
    hyd = batch.mode_trace(HYD, modes, capacity=1)
    bar = batch.mode_trace(BAR, modes, capacity=1, lb_hydrovars=True)
    hyd.sample(); bar.sample()
    steps, a_hyd = hyd.read()
    assert steps.tolist() == [[5, 1005, 5]] and a_hyd.shape == (1, 3, 3, 5)
    a_bar = bar.read()[1]
    for r, v in enumerate(batch.replicas):
        _check_record(pkg, a_hyd[0, r], v.LBM_hydrovars()[_index(pkg, HYD, False)], n, modes, tables, (n, schedule, "hydrovs", r))
        _check_record(pkg, a_bar[0, r], v.LBM_hydrovars_density()[_index(pkg, BAR, True)], n, modes, tables, (n, schedule, "hydrovsbar", r))
    batch.close()


# ---- 3. independence ----------------------------------------------------------------------------------------------------------
def test_a_replica_records_the_bits_of_the_lattice_run_alone(pkg):
    """Replica r of a B = 3 batch against the same lattice alone; a moments trace and a spectrum trace attached before, an
    interface trace and a spectrum trace after (an owner carries one moments trace); every = 1 and 3 at the common steps;
    two mode traces on one owner."""
    n = (13, 10, 6)
    modes = ms.issue_modes(n)
    batch = _batch(pkg, n, "fused")
    before = [batch.trace(every=1, capacity=8), batch.spectrum_trace([(0, 0)], every=1, capacity=8)]
    fine = batch.mode_trace(HYD, modes, every=1, capacity=8)
    coarse = batch.mode_trace(HYD, modes, every=3, capacity=2)
    after = [batch.interface_trace(0.5, field="rho", every=2, capacity=4), batch.spectrum_trace([(0, 1)], every=1, capacity=8)]
    fine.sample(); fine.sample()
    batch.LBM_timestep(6)
    fs, fa = fine.read()
    cs, ca = coarse.read()
    assert fa.shape == (8, 3, 3, 5) and np.array_equal(fa[0], fa[1]) and np.abs(fa[0]).max() > 0
    assert np.array_equal(cs, fs[[4, 7]]) and np.array_equal(ca, fa[[4, 7]])        # steps 3 and 6 of both
    assert not np.array_equal(fa[4], fa[7])
    for t in before + after:
        assert t.count in (3, 6)
    batch.close()
    for r, p in enumerate(_params()):
        lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lbm.LBM_init_mixture()
        if r == 1:
            lbm.set_steps_done(1000)
        alone = lbm.mode_trace(HYD, modes, every=1, capacity=8)
        alone.sample(); alone.sample()
        for _ in range(6):
            lbm.LBM_timestep(1)
        steps, amp = alone.read()
        assert np.array_equal(steps[:, 0], fs[:, r]) and np.array_equal(amp[:, 0], fa[:, r]), r
        # a window of the record
        s2, a2 = alone.read(first=3, count=2)
        assert np.array_equal(s2, steps[3:5]) and np.array_equal(a2, amp[3:5])
        lbm.close()


# ---- 4. lifecycle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n = (9, 7, 5)
    modes = np.array([(1, 0, 0), (0, 1, 1)])
    o = _lone(pkg, n) if owner == "lone" else _batch(pkg, n)
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: max(v.steps_done for v in o.replicas) - 1000)
    other = o.trace(every=1, capacity=16)
    tr = o.mode_trace(["rho"], modes, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="mode trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0
    assert tr.count == 1 and tr.read()[0][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(7)
    assert done() == 7 and tr.count == 3 and other.count == 7
    state = [u.copy() for u in o.populations()]
    with pytest.raises(pkg.BflbmError, match="mode trace full"):
        o.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="mode trace full"):
        tr.sample()
    assert done() == 7 and tr.count == 3 and other.count == 7
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps, amp = tr.read()
    assert (steps[:, 0] - steps[0, 0]).tolist() == [0, 2, 4] and steps[0, 0] == 2
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                      # the every-counter restarted: steps 8, 9 sample at 9
    assert tr.count == 1 and tr.read()[0][0, 0] == 9
    # the owner goes first: the trace stays readable with the same bits, refuses a sample, closes twice
    steps, amp = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, amp2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(amp, amp2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    one = [(1, 0, 0)]
    lbm, batch = _lone(pkg, n), _batch(pkg, n)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_modes_create.*replica of a batch.*use bflbm_batch_modes_create"):
        batch.replicas[0].mode_trace([0], one)
    for owner, call in ((lbm, "bflbm_modes_create"), (batch, "bflbm_batch_modes_create")):
        nrep = 1 if owner is lbm else 3
        for pattern, variables, modes, kw in (("variable index 22 outside hydrovs", [0, 22], one, {}),
                                              ("variable index -1 outside hydrovs", [-1], one, {}),
                                              ("variable index 9 outside hydrovsbar", [9], one, dict(lb_hydrovars=True)),
                                              ("variable index 3 given twice", [3, 1, 3], one, {}),
                                              ("1..8 variables", list(range(9)), one, {}),
                                              ("1..8 variables", [], one, {}),
                                              ("1..64 wavevectors", [0], [(k, 0, 0) for k in range(65)], {}),
                                              ("1..64 wavevectors", [0], np.zeros((0, 3), dtype=np.int64), {}),
                                              ("every must be >= 1", [0], one, dict(every=0)),
                                              ("capacity must be >= 1", [0], one, dict(capacity=0)),
                                              ("exceeds 1 TB", [0], one, dict(capacity=(1 << 37) // (2 * nrep) + 1))):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                owner.mode_trace(variables, modes, **kw)
            assert call in str(e.value)
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        full = owner.mode_trace(list(range(8)), [(k, -k, 2 * k) for k in range(64)], capacity=1)      # the limits themselves
        full.sample()
        assert np.isfinite(full.read()[1].view(np.float64)).all()
        full.close()
    with pytest.raises(ValueError):
        lbm.mode_trace(["no_such_variable"], one)
    with pytest.raises(ValueError):
        lbm.mode_trace([0], [(1.5, 0, 0)])
    with pytest.raises(ValueError):
        lbm.mode_trace([0], [1, 0, 0])
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_modes_create inside an open step"):
        lbm.mode_trace([0], one)
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.mode_trace([0], one, capacity=2)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [1, 2]       # the split step samples in its finish
    lbm.close(); batch.close()
    # a box whose x and y tables do not fit the projection kernel
    wide = pkg.BinaryLBM(4700, 8, 4)
    with pytest.raises(pkg.BflbmError, match="bflbm_modes_create.*phase tables.*LDS"):
        wide.mode_trace([0], one)
    wide.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_modes_create.*nranks > 1"):
        slab.mode_trace([0], one)
    slab.close()


def test_mode_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lone(pkg, (9, 7, 5))
    t = ctypes.c_void_p()
    va, mo = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 6)(1, 0, 0, 0, -1, 2)
    check(lib.bflbm_modes_create(lbm._h, 2, va, 1, 2, mo, 1, 4, ctypes.byref(t)))
    lbm.LBM_timestep(3)

    def read(first, count):
        amp, steps = np.empty((count, 1, 2, 2), dtype=np.complex128), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_modes_read(t, first, count, amp.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.c_void_p)))
        return steps, amp
    steps0, amp0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3]
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    steps1, amp1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(amp0, amp1)
    assert np.array_equal(read(2, 1)[1][0], amp0[2])       # a window
    assert lib.bflbm_modes_read(t, 2, 2, amp0.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.bflbm_modes_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_modes_destroy(t))


# ---- 5. sign and scale on a physical state ---------------------------------------------------------------------------------------
def _planted_shear(pkg, ob, tau, n=16, amp=1e-4):
    lbm = pkg.BinaryLBM(n, n, n, params=pkg.default_params(kBT=0.0, alpha0=0.0, tau_f=tau, tau_g=tau))
    lbm.LBM_init(*rc.shear_wave_state(ob, n, n, n, amp))
    return lbm


def test_sign_and_scale_of_a_planted_shear_wave(pkg, ob):
    """f_i = g_i = w_i (1 + 3 c_iy A sin(2 pi x / 16)): frame 0 of hydrovsbar ufy at (1, 0, 0) is -i A N / 2.  The CPU
    oracle gives a deviation of 3e-14 of A N / 2; the bound is 1e-9."""
    A, N = 1e-4, 16 ** 3
    lbm = _planted_shear(pkg, ob, 1.0)
    tr = lbm.mode_trace(["ufy"], [(1, 0, 0)], capacity=1, lb_hydrovars=True)
    tr.sample()
    a = tr.read()[1][0, 0, 0, 0]
    print("a^ / (A N / 2) = %r" % (a / (A * N / 2)))
    assert abs(a.real) <= 1e-9 * A * N / 2 and abs(a.imag + A * N / 2) <= 1e-9 * A * N / 2
    lbm.close()


# ---- 6. Onsager regression -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_thermal_modes_relax_like_a_planted_one(pkg, ob, tau):
    """8 x 16^3 mixtures, alpha0 = 0, kBT = 1e-5, seeds 1234..1241, 200 steps discarded, 1500 sampled every step:
    A = u^f + u^g of hydrovsbar at (1,0,0), (0,1,0), (0,0,1), the six transverse (axis, component) pairs;
    C(s) = mean over t and the pairs of Re(A(t + s) conj A(t)) per replica.  Against r(s) = |A(s)| / |A(0)| of the planted
    shear wave of the test above.  The CPU oracle with 4 replicas (seeds 1234..1237):
        tau 1:    C(10)/C(0) = 0.619 +- 0.007 (r = 0.631), C(20)/C(0) = 0.369 +- 0.012 (r = 0.386)
        tau 1/2:  C(10)/C(0) = 0.764 +- 0.008 (r = 0.773), C(20)/C(0) = 0.585 +- 0.015 (r = 0.598)
    On an MI355X, 8 replicas: tau 1: 0.629 +- 0.007 (r = 0.631) and 0.381 +- 0.009 (r = 0.386); tau 1/2: 0.772 +- 0.006
    (r = 0.773) and 0.595 +- 0.010 (r = 0.598).
    u_f alone gives 0.31 at tau 1, lag 10: half of its variance is the fast relative motion of the two fluids."""
    n = (16, 16, 16)
    modes = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1)])
    batch = pkg.BatchLBM(n, params=dict(alpha0=0.0, kBT=1e-5, tau_f=tau, tau_g=tau), seeds=list(range(1234, 1242)), replicas=8)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.LBM_timestep(200)
    tr = batch.mode_trace(["ufx", "ufy", "ufz", "ugx", "ugy", "ugz"], modes, every=1, capacity=1500, lb_hydrovars=True)
    batch.LBM_timestep(1500)
    steps, amp = tr.read()
    batch.close()
    assert amp.shape == (1500, 8, 6, 3) and steps[0].tolist() == [201] * 8 and steps[-1].tolist() == [1700] * 8
    A = amp[:, :, 0:3] + amp[:, :, 3:6]                    # [t, replica, component, axis of the wavevector]
    C = pkg.analysis.time_correlation(A, max_lag=20).real
    transverse = ~np.eye(3, dtype=bool)
    C = C[:, :, transverse].mean(axis=-1)                  # [lag, replica]
    # the planted mode
    lbm = _planted_shear(pkg, ob, tau)
    det = lbm.mode_trace(["ufy", "ugy"], [(1, 0, 0)], every=1, capacity=21, lb_hydrovars=True)
    det.sample()
    lbm.LBM_timestep(20)
    d = det.read()[1][:, 0].sum(axis=1)[:, 0]
    lbm.close()
    r = np.abs(d) / np.abs(d[0])
    for s in (10, 20):
        ratio = C[s] / C[0]
        mean, se = ratio.mean(), ratio.std(ddof=1) / np.sqrt(len(ratio))
        print("tau %g lag %d: thermal C(s)/C(0) = %.4f +- %.4f, deterministic r(s) = %.4f" % (tau, s, mean, se, r[s]))
        assert se <= 0.02, (tau, s, se)
        assert abs(mean - r[s]) <= 0.04, (tau, s, mean, r[s])


# ---- 7. the shear wave through the trace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.5, 0.8])
def test_shear_wave_viscosity_through_the_trace(pkg, ob, tau):
    """The setup of tests/test_gpu_relaxation.py::test_shear_wave_decays_with_viscosity_cs2_tau and its bound."""
    n = (64, 8, 8)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(tau_f=tau, tau_g=tau, alpha0=0.0))
    lbm.LBM_init(*rc.shear_wave_state(ob, *n))
    tr = lbm.mode_trace(["ufy"], [(1, 0, 0)], every=100, capacity=3, lb_hydrovars=True)
    lbm.LBM_timestep(300)
    steps, amp = tr.read()
    assert steps[:, 0].tolist() == [100, 200, 300]
    a = np.abs(amp[:, 0, 0, 0])
    nu = -np.log(a[2] / a[0]) / ((2 * np.pi / n[0]) ** 2 * 200)
    print("tau %g: nu / (cs2 tau) = %.6f" % (tau, nu / (tau / 3.0)))
    assert abs(nu / (tau / 3.0) - 1.0) < 5e-3, nu
    ufy = lbm.LBM_hydrovars_density()[3]
    host = pkg.analysis.fourier_modes(ufy, [(1, 0, 0)])[0]
    lim = ms.depth_bound(*n) * np.abs(ufy).sum()
    print("|A(300)| device %.17g host %.17g, difference / (depth_bound sum |a|) = %.3g" % (a[2], abs(host), abs(a[2] - abs(host)) / lim))
    assert abs(a[2] - abs(host)) <= lim
    lbm.close()
