"""GPU: spectrum traces (SpectrumTrace, bflbm_spectrum_*): the structure factor of pairs of hydrodynamic variables of
every sample, binned into shells in |q| or into |k| along one axis, recorded on the device.

The definition is in include/bflbm.h ("Spectrum traces"); analysis.spectrum_bins / binned_spectrum restate it in numpy.
Tolerance of every spectral comparison, from the bar of tests/test_gpu_structfact.py (two FFT libraries agree to 1e-11 of
the pair's largest |S(k)|): a bin adds count[bin] modes, so
    |device - numpy| <= 1e-11 count[bin] max_k |S_ab(k)|        per bin and pair,
with the maximum over the full numpy spectrum of that sample.  The k = 0 mode counts in that maximum also where zero_avg
leaves it out of bin 0: the rounding error of a transform scales with the 2-norm of the field, to which the mean
contributes, and it lands in every mode.  (A uniform field is the plain case: right after LBM_init_mixture every mode but
k = 0 is exactly zero, numpy returns zeros and dust of 1e-30 there, hipFFT returns dust of 1e-29 on sizes that are no power
of two, and both are right to 1e-30 of S(0).)
The shapes: odd nx (no Nyquist plane) with odd ny and nz and nz < 8, an anisotropic box whose W is decided by the lcm, a
padded pitch, and a cube."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 16), (12, 10, 14), (9, 7, 5), (8, 32, 16)]
KINDS = ["shell", "x", "y", "z"]
TRIO = [(0, 0), (1, 1), (0, 1)]                           # rho-rho, phi-phi, rho-phi


def _same(a, b):
    """Equal doubles, NaNs matched by position."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _host(pkg, fields, pairs, kinds, zero_avg=True, scale=None):
    """{kind: (sums[npairs, nbins] of analysis.binned_spectrum, tolerance[npairs, nbins])} of fields[ncomp, nz, ny, nx]."""
    n = fields.shape[:0:-1]
    hat = {}
    largest, rest = [], []
    for p, (a, b) in enumerate(pairs):
        for v in (a, b):
            if v not in hat:
                hat[v] = np.fft.fftn(fields[v])
        s = ((1.0 if scale is None else scale[p]) * hat[a] * np.conj(hat[b])).real / fields[a].size
        largest.append(np.abs(s).max())                    # over the full spectrum, k = 0 included (see the module's docstring)
        s[0, 0, 0] = 0.0
        rest.append(np.abs(s).max())                       # printed only: the same without the k = 0 mode
    out = {}
    for kind in kinds:
        count = pkg.analysis.spectrum_bins(n, kind, zero_avg)[1]
        sums = np.stack([pkg.analysis.binned_spectrum(fields[a], fields[b], kind, zero_avg, 1.0 if scale is None else scale[p])
                         for p, (a, b) in enumerate(pairs)])
        out[kind] = (sums, 1e-11 * count[None, :] * np.array(largest)[:, None], 1e-11 * count[None, :] * np.array(rest)[:, None])
    return out


def _close(dev, want, what):
    sums, tol, tol_rest = want
    err = np.abs(dev - sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst, worst_rest = [np.nanmax(np.where(t > 0, err / t, np.where(err > 0, np.inf, 0.0))) for t in (tol, tol_rest)]
    print(what, "worst |device - numpy| / tolerance = %.3g (%.3g of a tolerance without the k = 0 mode)" % (worst, worst_rest))
    assert dev.shape == sums.shape and np.isfinite(dev).all(), what
    assert np.all(err <= tol), (what, worst)


def _lone(pkg, n, schedule=None, **params):
    p = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0)  # test_device_structure_factor_matches_host's mixture
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_mixture()
    return lbm


def _params():
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


def _batch(pkg, n, schedule=None):
    """The three replicas of tests/test_gpu_batch_structfact.py: they differ in parameters, seed and step counter."""
    batch = pkg.BatchLBM(n, params=_params(), schedule=schedule)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    return batch


# ---- 1. geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_bins_equal_the_restatement(pkg, n):
    lbm = _lone(pkg, n)
    batch = _batch(pkg, n)
    for kind in KINDS:
        for zero_avg in (True, False):
            for owner in (lbm, batch):
                tr = owner.spectrum_trace(TRIO, kind=kind, zero_avg=zero_avg, capacity=1)
                _, want_count, want_q = pkg.analysis.spectrum_bins(n, kind, zero_avg)
                count, q = tr.bins()
                assert count.dtype == np.int64 and np.array_equal(count, want_count), (kind, zero_avg)
                assert np.array_equal(np.isnan(q), np.isnan(want_q))
                ok = ~np.isnan(q)
                assert np.all(np.abs(q[ok] - want_q[ok]) <= 1e-14 * np.abs(want_q[ok])), (kind, zero_avg)
                nbins, npairs, nchunks, most = tr.geometry()
                assert nbins == len(want_count) and npairs == 3
                assert most >= 1 and np.count_nonzero(count) <= nchunks <= nbins * most
                assert count.sum() == n[0] * n[1] * n[2] - (1 if zero_avg else 0)
                tr.close()
    lbm.close(); batch.close()


# ---- 2. a lone context ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_lone_spectrum_trace_matches_host(pkg, n):
    lbm = _lone(pkg, n)
    names = pkg.plotfile.variable_names(22)
    lbm.LBM_timestep(15)
    traces = {kind: lbm.spectrum_trace(names, kind=kind, every=5, capacity=4) for kind in KINDS}    # an owner may carry several
    pairs = traces["shell"].pairs
    assert len(pairs) == 22 and traces["x"].pair_names() == pkg.structfact.StructFact(names).pair_names()
    want = []
    for _ in range(3):
        lbm.LBM_timestep(5)
        want.append(_host(pkg, lbm.LBM_hydrovars(), pairs, KINDS))
    for kind, tr in traces.items():
        steps, sums = tr.read()
        nbins = tr.geometry()[0]
        assert steps.dtype == np.int64 and steps[:, 0].tolist() == [20, 25, 30] and sums.shape == (3, 1, 22, nbins)
        for s in range(3):
            _close(sums[s, 0], want[s][kind], (n, kind, "step", 20 + 5 * s))
        count = tr.bins()[0]
        mean = tr.mean()
        assert _same(mean[:, :, :, count > 0], (sums / np.where(count > 0, count, 1))[:, :, :, count > 0])
        assert np.isnan(mean[..., count == 0]).all() and count[0] == (0 if kind == "shell" else count[0])
    # auto-correlations are sums of squares
    auto = [i for i, (a, b) in enumerate(pairs) if a == b]
    assert np.all(traces["shell"].read()[1][:, 0, auto] >= 0)
    lbm.close()


# ---- 3. a batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("n", SHAPES)
def test_batch_spectrum_trace_matches_host(pkg, n, schedule):
    batch = _batch(pkg, n, schedule)
    views = batch.replicas
    names = pkg.plotfile.variable_names(22)
    traces = {kind: batch.spectrum_trace(names, kind=kind, every=1, capacity=8) for kind in KINDS}
    pairs = traces["shell"].pairs
    for tr in traces.values():
        tr.sample()                                        # k = 0 right after the inits: the device records are stale
    want = {0: [_host(pkg, v.LBM_hydrovars(), pairs, KINDS) for v in views]}
    done = 0
    for nsteps in (1, 1, 5):                               # after 1, 2 and 7 steps: both parities of k
        batch.LBM_timestep(nsteps)
        done += nsteps
        want[done] = [_host(pkg, v.LBM_hydrovars(), pairs, KINDS) for v in views]
    for kind, tr in traces.items():
        steps, sums = tr.read()
        assert sums.shape == (8, 3, 22, tr.geometry()[0])
        assert steps.tolist() == [[s, 1000 + s, s] for s in range(8)]
        for s, per_replica in want.items():
            for r in range(3):
                _close(sums[s, r], per_replica[r][kind], (n, schedule, kind, "step", s, "replica", r))
    batch.close()


# ---- 4. hydrovsbar ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_spectrum_trace_of_hydrovsbar(pkg, n):
    names = pkg.plotfile.variable_names(9)
    batch = _batch(pkg, n)
    views = batch.replicas
    batch.LBM_timestep(3)
    before = [v.LBM_hydrovars() for v in views]
    traces = {kind: batch.spectrum_trace(names, kind=kind, lb_hydrovars=True, capacity=2) for kind in KINDS}
    pairs = traces["shell"].pairs
    assert pairs == pkg.structfact.StructFact(names).pairs and all(max(p) < 9 for p in pairs)
    for tr in traces.values():
        tr.sample()
    for v, h in zip(views, before):
        assert np.array_equal(v.LBM_hydrovars(), h)        # a sample changes nothing a view observes
    want = [_host(pkg, v.LBM_hydrovars_density(), pairs, KINDS) for v in views]
    for kind, tr in traces.items():
        sums = tr.read()[1]
        for r in range(3):
            _close(sums[0, r], want[r][kind], (n, kind, "replica", r))
    batch.close()
    # a lone context, with a scale per pair and the k = 0 mode kept
    lbm = _lone(pkg, n)
    lbm.LBM_timestep(4)
    scale = [1.0 + 0.25 * p for p in range(len(pairs))]
    tr = lbm.spectrum_trace(names, kind="shell", lb_hydrovars=True, zero_avg=False, var_scaling=scale, capacity=1)
    tr.sample()
    _close(tr.read()[1][0, 0], _host(pkg, lbm.LBM_hydrovars_density(), pairs, ["shell"], zero_avg=False, scale=scale)["shell"], (n, "lone"))
    lbm.close()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------
def _run_with_two_traces(pkg, make, step):
    owner = make()
    names = pkg.plotfile.variable_names(22)
    fine = owner.spectrum_trace(names, kind="shell", every=1, capacity=8)
    coarse = owner.spectrum_trace(names, kind="shell", every=2, capacity=3)
    fine.sample(); fine.sample()
    step(owner, 6)
    out = fine.read(), coarse.read()
    owner.close()
    return out


@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_records_are_deterministic(pkg, owner):
    n = (12, 10, 14)
    make = (lambda: _lone(pkg, n)) if owner == "lone" else (lambda: _batch(pkg, n))
    (fs, fine), (cs, coarse) = _run_with_two_traces(pkg, make, lambda o, k: o.LBM_timestep(k))
    assert fine.shape[0] == 8 and coarse.shape[0] == 3
    assert np.array_equal(fine[0], fine[1]) and np.abs(fine[0]).max() > 0           # the same state sampled twice
    assert np.array_equal(cs, fs[[3, 5, 7]]) and np.array_equal(coarse, fine[[3, 5, 7]])    # steps 2, 4, 6 of both
    assert not np.array_equal(fine[3], fine[5])
    (fs2, fine2), (cs2, coarse2) = _run_with_two_traces(pkg, make, lambda o, k: [o.LBM_timestep(1) for _ in range(k)])
    assert np.array_equal(fs, fs2) and np.array_equal(fine, fine2) and np.array_equal(coarse, coarse2)   # a second owner


# ---- 6. bins that span several chunks -----------------------------------------------------------------------------------------
# A chunk holds at most 2048 half-spectrum entries.  An axis bin of a cubic n^3 box holds n^2 of them, so 65 is the
# smallest n at which an axis bin takes 3 chunks (65^2 = 4225 > 4096 >= 64^2); the largest shells do so before.
@pytest.mark.parametrize("kind", ["shell", "x"])
def test_bins_that_span_several_chunks(pkg, kind):
    for n, least in ((65, 3), (64, 2)):
        probe = pkg.BinaryLBM(n, n, n)
        tr = probe.spectrum_trace(TRIO, kind="x", capacity=1)
        assert tr.geometry()[3] == least, (n, tr.geometry())
        probe.close()
    n = (65, 65, 65)
    lbm = _lone(pkg, n)
    names = pkg.plotfile.variable_names(22)
    lbm.LBM_timestep(15)
    tr = lbm.spectrum_trace(names, kind=kind, every=5, capacity=3)
    nbins, npairs, nchunks, most = tr.geometry()
    assert most >= 3 and nchunks > nbins, tr.geometry()
    for s in range(3):
        lbm.LBM_timestep(5)
        want = _host(pkg, lbm.LBM_hydrovars(), tr.pairs, [kind])[kind]
        steps, sums = tr.read()
        assert steps[:, 0].tolist() == [20, 25, 30][:s + 1]
        _close(sums[s, 0], want, (n, kind, "step", 20 + 5 * s))
    lbm.close()


# ---- 7. the axes are not confused ------------------------------------------------------------------------------------------------
def test_a_stripe_shows_on_its_own_axis_only(pkg):
    n = (8, 16, 24)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(kBT=0.0))
    lbm.LBM_init_stripe(0.5)
    traces = {kind: lbm.spectrum_trace(TRIO, kind=kind, capacity=1) for kind in ("x", "y", "z")}
    for tr in traces.values():
        tr.sample()                                        # frame 0
    want = _host(pkg, lbm.LBM_hydrovars(ncomp=2), TRIO, ["x", "y", "z"])
    for kind, tr in traces.items():
        sums = tr.read()[1][0, 0]
        tol = want[kind][1]
        assert np.all(tol[:, 1:] > 0)
        _close(sums, want[kind], (n, kind))
        if kind == "z":
            assert np.any(np.abs(sums[:, 1:]) > 1000 * tol[:, 1:])
        else:
            assert np.all(np.abs(sums[:, 1:]) <= tol[:, 1:]), kind
    lbm.close()


# ---- 8. the trace changes nothing ------------------------------------------------------------------------------------------------
def _watched(pkg, owner, with_spectrum):
    names = pkg.plotfile.variable_names(22)
    recs = [owner.trace(every=1, capacity=13), owner.interface_trace(0.5, field="rho", every=1, capacity=13)]
    spec = []
    if with_spectrum:                                      # created between the two: served between them after a step
        spec = [owner.spectrum_trace(names, kind="shell", every=1, capacity=13),
                owner.spectrum_trace(pkg.plotfile.variable_names(9), kind="z", lb_hydrovars=True, every=1, capacity=13)]
    recs.append(owner.interface_trace(0.5, field="phi", every=3, capacity=4))
    return recs, spec


def _unchanged(pkg, make, pops, counters):
    a, b = make(), make()
    recs_a, spec = _watched(pkg, a, True)
    recs_b, _ = _watched(pkg, b, False)
    for _ in range(4):
        a.LBM_timestep(3); b.LBM_timestep(3)
    assert counters(a) == counters(b)
    for u, v in zip(pops(a), pops(b)):
        assert np.array_equal(u, v)
    for ra, rb in zip(recs_a, recs_b):
        (sa, va), (sb, vb) = ra.read(), rb.read()
        assert np.array_equal(sa, sb) and _same(va, vb) and sa.shape[0] in (4, 12)
    for tr in spec:
        steps, sums = tr.read()
        assert steps.shape[0] == 12 and np.isfinite(sums).all() and np.abs(sums).max() > 0
    a.LBM_timestep(1); b.LBM_timestep(1)                   # the step after the last sample
    for u, v in zip(pops(a), pops(b)):
        assert np.array_equal(u, v)
    a.close(); b.close()


@pytest.mark.parametrize("n,schedule", [((12, 10, 14), "two_pass"), ((12, 10, 14), "fused"), ((64, 8, 12), "handover")])
def test_a_spectrum_trace_changes_nothing_lone(pkg, n, schedule):
    def make():
        lbm = _lone(pkg, n, schedule)
        if schedule == "handover":
            assert lbm.resolved_schedule() == "handover"
        return lbm
    _unchanged(pkg, make, lambda o: o.populations(), lambda o: o.steps_done)


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_a_spectrum_trace_changes_nothing_batch(pkg, schedule):
    _unchanged(pkg, lambda: _batch(pkg, (12, 10, 14), schedule), lambda o: o.populations(), lambda o: [v.steps_done for v in o.replicas])


# ---- 9. lifecycle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    """every = 2, capacity = 3 (the protocol of tests/test_gpu_trace.py): 7 steps add the samples of steps 2, 4 and 6; an
    eighth does not fit."""
    n = (9, 7, 5)
    o = _lone(pkg, n) if owner == "lone" else _batch(pkg, n)
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: max(v.steps_done for v in o.replicas) - 1000)
    tr = o.spectrum_trace(TRIO, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="spectrum trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0                   # refused whole: nothing stepped, nothing recorded
    o.LBM_timestep(7)
    assert done() == 7 and tr.count == 3
    state = [u.copy() for u in o.populations()]
    with pytest.raises(pkg.BflbmError, match="spectrum trace full"):
        o.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="spectrum trace full"):
        tr.sample()
    assert done() == 7 and tr.count == 3
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps, sums = tr.read()
    assert (steps[:, 0] - steps[0, 0]).tolist() == [0, 2, 4]
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                      # the every-counter restarted: steps 8, 9 sample at 9
    assert tr.count == 1 and tr.read()[0][0, 0] == steps[0, 0] + 7
    # the owner goes first: the trace stays readable with the same bits, refuses a sample, closes twice
    steps, sums = tr.read()
    bins, geo = tr.bins(), tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, sums2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(sums, sums2)
    assert tr.geometry() == geo and all(_same(u, v) for u, v in zip(bins, tr.bins()))
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm, batch = _lone(pkg, n), _batch(pkg, n)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_spectrum_create.*replica of a batch.*bflbm_batch_spectrum_create"):
        batch.replicas[0].spectrum_trace(TRIO)
    for owner, call in ((lbm, "bflbm_spectrum_create"), (batch, "bflbm_batch_spectrum_create")):
        for pattern, pairs, kw in (("variable index 22 outside hydrovs", [(0, 22)], {}),
                                   ("variable index -1 outside hydrovs", [(-1, 0)], {}),
                                   ("variable index 9 outside hydrovsbar", [(0, 9)], dict(lb_hydrovars=True)),
                                   ("kind must be", TRIO, dict(kind=4)),
                                   ("every must be >= 1", TRIO, dict(every=0)),
                                   ("capacity must be >= 1", TRIO, dict(capacity=0)),
                                   ("1..32 pairs", [(0, 0)] * 33, {}),
                                   ("1..32 pairs", [], {})):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                owner.spectrum_trace(pairs, **kw)
            assert call in str(e.value)
        assert not getattr(owner, "_dependents", [])       # nothing was attached
    with pytest.raises(ValueError):
        lbm.spectrum_trace(TRIO, kind="w")
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_spectrum_create inside an open step"):
        lbm.spectrum_trace(TRIO)
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.spectrum_trace(TRIO, capacity=2)
    lbm.step_boundary()
    for call in (tr.sample, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 1 and tr.read()[0][0, 0] == 2       # the split step samples in its finish
    lbm.close(); batch.close()


def test_spectrum_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lone(pkg, (9, 7, 5))
    t = ctypes.c_void_p()
    a, b = (ctypes.c_int * 3)(0, 1, 0), (ctypes.c_int * 3)(0, 1, 1)
    check(lib.bflbm_spectrum_create(lbm._h, 3, a, b, None, 1, 0, 1, 1, 4, ctypes.byref(t)))
    lbm.LBM_timestep(3)
    nbins = ctypes.c_int()
    check(lib.bflbm_spectrum_geometry(t, ctypes.byref(nbins), None, None, None))

    def read(first, count):
        sums, steps = np.empty((count, 1, 3, nbins.value)), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_spectrum_read(t, first, count, sums.ctypes.data_as(ctypes.c_void_p), steps.ctypes.data_as(ctypes.c_void_p)))
        return steps, sums
    steps0, sums0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3]
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    steps1, sums1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(sums0, sums1)
    assert np.array_equal(read(2, 1)[1][0], sums0[2])      # a window
    assert lib.bflbm_spectrum_read(t, 2, 2, sums0.ctypes.data_as(ctypes.c_void_p), None) != 0
    assert lib.bflbm_spectrum_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_spectrum_destroy(t))


# ---- 10. spinodal growth --------------------------------------------------------------------------------------------------------
def test_spinodal_domains_grow(pkg):
    """24^3 mixture, alpha0 = 2.5, kBT = 1e-5, 200 steps sampled every 10: S = S_rr + S_pp - 2 S_rp is the spectrum of
    rho - phi.  The CPU oracle (which the exact schedules reproduce bit for bit) gives L = 3.59, 4.88, ..., 10.45 at step
    100, ..., 17.29 at step 200 and the peak bin 5, 5, 5, 5, 4, 4, 3, 3, 2, ..., 1; asserted are the two orderings."""
    n = (24, 24, 24)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.5, kBT=1e-5), schedule="fused")
    lbm.LBM_init_mixture()
    tr = lbm.spectrum_trace(TRIO, kind="shell", every=10, capacity=20, lb_hydrovars=True)
    count, q = tr.bins()
    host = []
    for _ in range(20):
        lbm.LBM_timestep(10)
        rho, phi = lbm.LBM_hydrovars_density(ncomp=2)
        host.append(pkg.analysis.binned_spectrum(rho - phi, rho - phi, "shell"))
    steps, mean = tr.read()[0], tr.mean()
    assert steps[:, 0].tolist() == list(range(10, 201, 10))
    S = mean[:, 0, 0] + mean[:, 0, 1] - 2 * mean[:, 0, 2]
    L = pkg.analysis.domain_length(q, S)
    print("L =", np.array2string(L, precision=2), "peak bin", np.nanargmax(S[:, 1:], axis=1) + 1)
    assert L.shape == (20,) and np.all(np.diff(L) > 0), L
    peak = np.nanargmax(S[:, 1:], axis=1) + 1
    assert np.all(np.diff(peak) <= 0) and peak[0] > peak[-1], peak
    with np.errstate(invalid="ignore", divide="ignore"):
        L_host = pkg.analysis.domain_length(q, np.where(count > 0, np.array(host) / count, np.nan))
    assert np.all(np.abs(L - L_host) <= 1e-9 * L_host), np.abs(L / L_host - 1).max()
    lbm.close()
