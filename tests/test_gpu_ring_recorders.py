"""GPU: recorders of a ring of z-slabs (RingLBM.trace, RingLBM.spectrum_trace; bflbm_ring_trace_create,
bflbm_ring_spectrum_create).  All rings live on device 0.

The moments trace of a ring adds in a lone context's order, so with the bit-exact schedules (and kBT = 1e-5, where the
ring's noise does not depend on the decomposition, tests/test_gpu_slabs.py) its records equal a lone lattice's bit for
bit.  The spectrum trace of a ring is a slab FFT with per-slab binning: it is compared with the numpy restatement
(analysis.binned_spectrum) under the tolerance of tests/test_gpu_spectrum.py, taken over from there with its helpers:
    |device - numpy| <= 1e-11 count[bin] max_k |S_ab(k)|        per bin and pair.
The profile and histogram traces of a ring have their definition tests in test_gpu_profile.py and test_gpu_hist.py; here
they meet what all four kinds that gather a block per slab onto slab 0 share, the reuse of those blocks at every = 1.
The shapes: the smallest ring (2 slabs of 4 planes), ragged slabs of 4 / 4 / 5 planes with ky rows split 2 / 2 / 2, a
padded pitch on 4 slabs, odd nx with ky rows split 2 / 2 / 3, and a box whose axis bins take 3 chunks on every slab."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_hist import CASES, _fields, _ranges
from test_gpu_spectrum import KINDS, TRIO, _close, _host, _lone

pytestmark = pytest.mark.gpu

MIXTURE = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0)      # the mixture of test_gpu_spectrum._lone


def _ring(pkg, nslabs, n, schedule=None, **params):
    p = dict(MIXTURE)
    p.update(params)
    ring = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**p), schedule=schedule)
    ring.LBM_init_mixture()
    return ring


# ---- 1. moments: bit identity with a lone lattice ---------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("nslabs,n", [(2, (8, 8, 8)), (3, (10, 6, 13)), (4, (70, 9, 16))])
def test_ring_trace_equals_lone_trace(pkg, nslabs, n, schedule):
    for threshold in (None, 0.06):
        par = dict(alpha0=2.5, kBT=1e-5, seed=7)
        ring = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**par), schedule=schedule)
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule=schedule)
        traces = []
        for o in (ring, lone):
            o.LBM_init_droplet(0.25)
            traces.append(o.trace(every=2, capacity=4, threshold=threshold))
            o.LBM_timestep(8)
        (rs, rrec), (ls, lrec) = traces[0].read(), traces[1].read()
        assert rs.shape == (4, 1) and rs[:, 0].tolist() == [2, 4, 6, 8] and rrec.shape == (4, 1, 12)
        assert np.array_equal(rs, ls) and np.array_equal(rrec, lrec), (threshold, rrec - lrec)
        print(nslabs, n, schedule, "threshold", threshold, "cells above it", rrec[:, 0, 11].tolist())
        if threshold is None:
            assert np.all(rrec[:, 0, 0] > 0)
            assert np.array_equal(rrec[-1, 0, :10], ring.droplet_moments()[:10])
            assert np.array_equal(rrec[..., 10], rrec[..., 0]) and np.all(rrec[..., 11] == n[0] * n[1] * n[2])
        ring.close()
        assert traces[0]._h is None                          # closing the ring closed its moments trace
        lone.close()


# ---- 2. spectrum against the restatement ---------------------------------------------------------------------------------
def _records(pkg, nslabs, n, host=True):
    """The run of test 2: {(variables, kind, zero_avg): (steps, sums, count, q)} of the samples after steps 20, 25, 30, and
    (host) what numpy computes from the gathered fields of the same states."""
    ring = _ring(pkg, nslabs, n)
    names = {"hydrovs": pkg.plotfile.variable_names(22), "hydrovsbar": pkg.plotfile.variable_names(9)}
    ring.LBM_timestep(15)
    traces = {(v, kind, z): ring.spectrum_trace(names[v], kind=kind, every=5, capacity=3, lb_hydrovars=(v == "hydrovsbar"), zero_avg=z)
              for v in names for kind in KINDS for z in (True, False)}
    pairs = {v: traces[(v, "shell", True)].pairs for v in names}
    assert len(pairs["hydrovs"]) == 22 and all(max(p) < 9 for p in pairs["hydrovsbar"])
    want = []
    for _ in range(3):
        ring.LBM_timestep(5)
        if not host:
            continue
        fields = {"hydrovs": ring.LBM_hydrovars(), "hydrovsbar": ring.LBM_hydrovars_density()}
        want.append({(v, z): _host(pkg, fields[v], pairs[v], KINDS, zero_avg=z) for v in names for z in (True, False)})
    got = {key: tr.read() + tr.bins() for key, tr in traces.items()}
    ring.close()
    return got, want


SPECTRUM_CASES = [(2, (8, 8, 8)), (3, (10, 6, 13)), (4, (16, 16, 16)), (3, (9, 7, 12))]


@pytest.mark.parametrize("nslabs,n", SPECTRUM_CASES)
def test_ring_spectrum_trace_matches_host(pkg, nslabs, n):
    got, want = _records(pkg, nslabs, n)
    for (v, kind, z), (steps, sums, count, q) in got.items():
        _, want_count, want_q = pkg.analysis.spectrum_bins(n, kind, z)
        assert count.dtype == np.int64 and np.array_equal(count, want_count), (v, kind, z)
        assert steps[:, 0].tolist() == [20, 25, 30] and sums.shape[:2] == (3, 1) and sums.shape[3] == len(want_count)
        for s in range(3):
            _close(sums[s, 0], want[s][(v, z)][kind], (nslabs, n, v, kind, "zero_avg", z, "step", 20 + 5 * s))


@pytest.mark.parametrize("nslabs,n", SPECTRUM_CASES)
def test_ring_bins_equal_a_lone_trace(pkg, nslabs, n):
    ring, lone = _ring(pkg, nslabs, n), _lone(pkg, n)
    for kind in KINDS:
        for z in (True, False):
            a, b = ring.spectrum_trace(TRIO, kind=kind, zero_avg=z, capacity=1), lone.spectrum_trace(TRIO, kind=kind, zero_avg=z, capacity=1)
            (ca, qa), (cb, qb) = a.bins(), b.bins()
            assert np.array_equal(ca, cb) and np.array_equal(qa, qb, equal_nan=True), (kind, z)
            assert np.array_equal(ca, pkg.analysis.spectrum_bins(n, kind, z)[1])
            ga, gb = a.geometry(), b.geometry()
            assert ga[:2] == gb[:2] and ga[2] >= gb[2] and 1 <= ga[3] <= gb[3]   # the same bins cut per slab
            a.close(); b.close()
    ring.close(); lone.close()


def test_ring_of_one_slab_is_the_lone_trace(pkg):
    n = (10, 6, 13)
    names = pkg.plotfile.variable_names(22)
    out = []
    for make in (lambda: _ring(pkg, 1, n), lambda: _lone(pkg, n)):
        o = make()
        sp = o.spectrum_trace(names, kind="shell", every=2, capacity=3)
        mo = o.trace(every=2, capacity=3)
        o.LBM_timestep(6)
        out.append(sp.read() + sp.bins() + sp.geometry() + mo.read())
        o.close()
    assert len(out[0]) == len(out[1]) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(out[0], out[1]))
    assert out[0][0][:, 0].tolist() == [2, 4, 6] and np.abs(out[0][1]).max() > 0


# ---- 3. several chunks per (slab, bin) -------------------------------------------------------------------------------------
def test_ring_bins_that_span_several_chunks(pkg):
    """(16, 128, 65) on 2 slabs, kind x: a slab holds 64 of the 128 ky rows, so its kx bin has 65 x 64 = 4160 entries,
    more than two chunks of 2048."""
    n = (16, 128, 65)
    ring = _ring(pkg, 2, n)
    names = pkg.plotfile.variable_names(22)
    ring.LBM_timestep(5)
    tr = ring.spectrum_trace(names, kind="x", capacity=1)
    nbins, npairs, nchunks, most = tr.geometry()
    assert most >= 3 and nbins == 9 and npairs == 22 and nchunks >= 2 * 3 * nbins, tr.geometry()
    tr.sample()
    steps, sums = tr.read()
    assert steps.tolist() == [[5]]
    _close(sums[0, 0], _host(pkg, ring.LBM_hydrovars(), tr.pairs, ["x"])["x"], (n, "x"))
    ring.close()


# ---- 4. the two transposes agree ---------------------------------------------------------------------------------------------
def test_collect_kernel_and_copies_move_the_same_doubles(tmp_path):
    """The (3, (10, 6, 13)) run of test 2 in two fresh processes (the switch is read once), with and without
    BFLBM_RING_COPY_FALLBACK=1: the gathering kernel and the strided copies give the same records bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import __graft_entry__ as ge, test_gpu_ring_recorders as t\n"
            "got, _ = t._records(ge.load_package(), 3, (10, 6, 13), host=False)\n"
            "np.savez(sys.argv[1], **{'%%s_%%s_%%d' %% k: v[1] for k, v in got.items()})\n"
            "print('SAVED', len(got))\n") % (root, os.path.join(root, "tests"))
    recs = []
    for tag, env in (("kernel", {}), ("copies", {"BFLBM_RING_COPY_FALLBACK": "1"})):
        path = str(tmp_path / (tag + ".npz"))
        out = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "SAVED 16" in out.stdout, (env, out.stdout[-500:], out.stderr[-1500:])
        recs.append(np.load(path))
    assert sorted(recs[0].files) == sorted(recs[1].files) and len(recs[0].files) == 16
    for key in recs[0].files:
        assert np.isfinite(recs[0][key]).all() and np.abs(recs[0][key]).max() > 0, key
        assert np.array_equal(recs[0][key], recs[1][key]), key


# ---- 5. determinism and reuse hazards ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hist_ranges(pkg, n):
    """{source: {variable: (lo, hi, bins)}} of test_gpu_hist.CASES, the ranges taken from a lone lattice of the rings'
    mixture after 5 steps (the probe run of test_gpu_hist.test_ring_record_equals_the_lone_record); once per shape."""
    probe = _lone(pkg, n, schedule="fused")
    probe.LBM_timestep(5)
    ranges = {s: _ranges(_fields(pkg, probe, s, list(CASES[s][0])), CASES[s][0]) for s in ("hydrovs", "noise")}
    probe.close()
    return ranges


def _plane_and_bin_traces(pkg, o, capacity=16):
    """The profile and histogram traces of _watched: a z profile (its finish reads every slab's planes) and an x profile
    with a pair each, the histograms of hydrovs (two pair blocks) and of the noise (one pair block)."""
    ranges = _hist_ranges(pkg, tuple(o.n))
    return [o.profile_trace(["rho", "phi", "afz"], [("rho", "phi")], axis="z", every=1, capacity=capacity),
            o.profile_trace(["rho", "ubx"], [("rho", "ubx")], axis="x", every=1, capacity=capacity),
            o.histogram_trace(ranges["hydrovs"], CASES["hydrovs"][1], every=1, capacity=capacity),
            o.histogram_trace(ranges["noise"], CASES["noise"][1], source="noise", every=1, capacity=capacity)]


def _watched(pkg, ring, capacity=16):
    """One recorder or more of every kind that gathers a block per slab onto slab 0, all at every = 1."""
    names = pkg.plotfile.variable_names(22)
    return [ring.trace(every=1, capacity=capacity),
            ring.spectrum_trace(names, kind="shell", every=1, capacity=capacity),
            ring.spectrum_trace(pkg.plotfile.variable_names(9), kind="z", lb_hydrovars=True, every=1, capacity=capacity)
            ] + _plane_and_bin_traces(pkg, ring, capacity)


def _read(tr):
    """(steps, records) of any kind: ProfileTrace.read() hands them out the other way round."""
    out = tr.read()
    return out[::-1] if type(tr).__name__ == "ProfileTrace" else out


def test_ring_records_are_deterministic(pkg):
    """every = 1: a slab's buffers of one sample are still being read by another slab's stream when the next sample is
    due.  One call of 12 steps against a second ring stepped one call per step; the same state sampled twice by hand.
    The profile and histogram records, the doubled hand samples first, are also a lone lattice's bit for bit (kBT = 1e-5
    and a bit-exact schedule, as in test_gpu_profile and test_gpu_hist), so a block copied to the wrong place shows even
    if every run copies it there."""
    nslabs, n = 3, (10, 6, 13)
    a, b = _ring(pkg, nslabs, n), _ring(pkg, nslabs, n)
    ra, rb = _watched(pkg, a), _watched(pkg, b)
    lone = _lone(pkg, n, schedule="fused")
    rl = _plane_and_bin_traces(pkg, lone)
    for tr in ra + rb + rl:
        tr.sample(); tr.sample()
    a.LBM_timestep(12)
    for _ in range(12):
        b.LBM_timestep(1)
    lone.LBM_timestep(12)
    for ta, tl in zip(ra[-len(rl):], rl):
        (sa, va), (sl, vl) = _read(ta), _read(tl)
        assert type(ta) is type(tl) and np.array_equal(sa, sl)
        assert np.array_equal(va[:2], vl[:2]), type(ta).__name__             # the doubled hand samples of the initial state
        assert np.array_equal(va, vl), type(ta).__name__                     # ... and every sample of the run
    lone.close()
    for ta, tb in zip(ra, rb):
        (sa, va), (sb, vb) = _read(ta), _read(tb)
        assert sa[:, 0].tolist() == [0, 0] + list(range(1, 13)) and np.array_equal(sa, sb)
        assert np.isfinite(va).all() and np.array_equal(va, vb)
        assert np.array_equal(va[0], va[1]) and np.abs(va[0]).max() > 0      # the same state sampled twice
        assert not np.array_equal(va[5], va[9])
    for tr in ra:
        tr.sample(); tr.sample()
        rec = _read(tr)[1]
        assert np.array_equal(rec[-1], rec[-2]) and np.array_equal(rec[-1], rec[-3])   # ... and again after the run
    a.close(); b.close()


# ---- 6. a recorder changes nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,schedule", [((10, 6, 13), "fused"), ((64, 8, 12), "handover")])
def test_ring_recorders_change_nothing(pkg, n, schedule):
    a, b = _ring(pkg, 3, n, schedule), _ring(pkg, 3, n, schedule)
    if schedule == "handover":
        assert all(s.resolved_schedule() == "handover" for s in a.slabs + b.slabs)
    recs = _watched(pkg, a)
    a.LBM_timestep(12); b.LBM_timestep(12)
    assert a.steps_done == b.steps_done == 12 and [s.steps_done for s in a.slabs] == [12, 12, 12]
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    for tr in recs:
        steps, rec = _read(tr)
        assert steps[:, 0].tolist() == list(range(1, 13)) and np.isfinite(rec).all() and np.abs(rec).max() > 0
    a.LBM_timestep(1); b.LBM_timestep(1)                     # the step after the last sample
    assert a.steps_done == b.steps_done == 13
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    a.close(); b.close()


# ---- 7. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_ring_overflow_is_refused_whole_and_reset_restarts(pkg):
    """every = 2, capacity = 3 (the protocol of tests/test_gpu_trace.py): 7 steps add the samples of steps 2, 4 and 6; an
    eighth does not fit."""
    ring = _ring(pkg, 2, (8, 8, 8))
    mo = ring.trace(every=2, capacity=3)
    sp = ring.spectrum_trace(TRIO, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_step: trace full"):
        ring.LBM_timestep(8)
    assert ring.steps_done == 0 and mo.count == 0 and sp.count == 0      # refused whole: nothing stepped, nothing recorded
    ring.LBM_timestep(7)
    assert ring.steps_done == 7 and mo.count == 3 and sp.count == 3
    state = [u.copy() for u in ring.populations()]
    before = mo.read(), sp.read()
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_step: trace full"):
        ring.LBM_timestep(1)
    mo.close()
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_step: spectrum trace full"):
        ring.LBM_timestep(1)
    with pytest.raises(pkg.BflbmError, match="spectrum trace full"):
        sp.sample()
    assert [s.steps_done for s in ring.slabs] == [7, 7] and sp.count == 3
    assert all(np.array_equal(u, v) for u, v in zip(state, ring.populations()))
    steps, sums = sp.read()
    assert steps[:, 0].tolist() == [2, 4, 6] and np.array_equal(steps, before[1][0]) and np.array_equal(sums, before[1][1])
    assert np.array_equal(before[0][0], steps)
    sp.reset()
    assert sp.count == 0 and sp.read()[1].shape[0] == 0
    ring.LBM_timestep(2)                                     # the every-counter restarted: steps 8, 9 sample at 9
    assert sp.count == 1 and sp.read()[0][0, 0] == 9
    # the ring goes first: the spectrum trace stays readable with the same bits, refuses a sample, closes twice
    steps, sums = sp.read()
    bins, geo = sp.bins(), sp.geometry()
    ring.close()
    assert sp._h is not None
    steps2, sums2 = sp.read()
    assert np.array_equal(steps, steps2) and np.array_equal(sums, sums2)
    assert sp.geometry() == geo and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(bins, sp.bins()))
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        sp.sample()
    sp.close(); sp.close()
    assert sp._h is None


def test_ring_creation_refusals(pkg):
    ring = _ring(pkg, 2, (8, 8, 8))
    mo = ring.trace(every=1, capacity=4)
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_trace_create: the owner already has a trace"):
        ring.trace(every=1, capacity=4)
    for pattern, pairs, kw in (("variable index 22 outside hydrovs", [(0, 22)], {}),
                               ("variable index 9 outside hydrovsbar", [(0, 9)], dict(lb_hydrovars=True)),
                               ("kind must be", TRIO, dict(kind=4)),
                               ("every must be >= 1", TRIO, dict(every=0)),
                               ("capacity must be >= 1", TRIO, dict(capacity=0)),
                               ("1..32 pairs", [], {})):
        with pytest.raises(pkg.BflbmError, match=pattern) as e:
            ring.spectrum_trace(pairs, **kw)
        assert "bflbm_ring_spectrum_create" in str(e.value)
    assert getattr(ring, "_dependents", []) == [mo]          # nothing else was attached
    # a slab handed to the lone calls is refused as before
    with pytest.raises(pkg.BflbmError, match=r"bflbm_trace_create: a slab of a decomposed lattice \(nranks > 1\); traces take a lone single-slab context or a batch"):
        ring.slabs[0].trace(every=1, capacity=1)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_spectrum_create: a slab of a decomposed lattice \(nranks > 1\); spectrum traces take a lone single-slab context or a batch"):
        ring.slabs[1].spectrum_trace(TRIO)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_iface_create: a slab of a decomposed lattice \(nranks > 1\); interface traces take"):
        ring.slabs[1].interface_trace(0.5)
    thin = _ring(pkg, 3, (8, 2, 12))
    with pytest.raises(pkg.BflbmError, match=r"bflbm_ring_spectrum_create: fewer rows \(ny = 2\) than slabs \(3\)"):
        thin.spectrum_trace(TRIO)
    thin.close()
    sp = ring.spectrum_trace(TRIO, capacity=4)
    ring.LBM_timestep(1)
    # inside a slab's open step (slabs stepped by hand serve nothing, and the ring's recorders refuse)
    ring.slabs[1].step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_spectrum_create inside an open step"):
        ring.spectrum_trace(TRIO)
    mo.close()
    with pytest.raises(pkg.BflbmError, match="bflbm_ring_trace_create inside an open step"):
        ring.trace(every=1, capacity=1)
    for call in (sp.sample, sp.reset, sp.read):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    ring.slabs[1].step_interior(); ring.slabs[1].step_finish()
    assert sp.count == 1 and sp.read()[0].tolist() == [[1]]
    ring.close()
