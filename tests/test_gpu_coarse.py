"""GPU: coarse traces (CoarseTrace, bflbm_coarse_*): the block sums of chosen hydrodynamic variables and of products of
them over a periodic window of the box, recorded on the device.

The rule and the order of the sums are in include/bflbm.h ("Coarse traces"); analysis.coarse_fields restates them in numpy
and tests/test_coarse_abi.py holds that twin to the site-by-site walk of tests/coarse_blocks.py.  Here the device record is
compared with the twin of the downloaded fields of the same state bit for bit: lone lattices and replicas of a batch, a
mixture at kBT = 1e-5 under the fused schedule after 5 steps."""
import math

import numpy as np
import pytest

import coarse_blocks as cb

pytestmark = pytest.mark.gpu

HYD = ["rho", "phi", "ufx"]                                # of hydrovs; NV = 3
HYD_PAIRS = [("rho", "phi"), ("ufx", "ufx")]
BAR = ["phi"]                                              # of hydrovsbar; NV = 1, no pairs
SEAM = cb.CASES[2]                                         # (10, 6, 13): the window through the seam on all three axes


def _mixture(pkg, n, schedule="fused", **params):
    p = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0, seed=77)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=schedule)
    lbm.LBM_init_mixture()
    return lbm


def _params():
    return [dict(alpha0=a, tau_f=1.0, tau_g=1.0, kBT=1e-5, seed=s) for a, s in zip((1.0, 0.5, 1.5), (101, 202, 303))]


def _batch(pkg, n, params=None, schedule="fused"):
    batch = pkg.BatchLBM(n, params=params or _params(), schedule=schedule)
    for v in batch.replicas:
        v.LBM_init_mixture()
    return batch


def _slots(names, pairs):
    return [(names.index(a), names.index(b)) for a, b in pairs]


def _index(pkg, names, bar=False):
    all_names = pkg.plotfile.variable_names(9 if bar else 22)
    return [all_names.index(v) for v in names]


def _want(pkg, lattice, origin, extent, block):
    """(hydrovs record, hydrovsbar record) of the lattice's downloaded fields by the numpy twin."""
    hyd = lattice.LBM_hydrovars()[_index(pkg, HYD)]
    bar = lattice.LBM_hydrovars_density()[_index(pkg, BAR, True)]
    an = pkg.analysis
    return an.coarse_fields(hyd, _slots(HYD, HYD_PAIRS), origin, extent, block), an.coarse_fields(bar, [], origin, extent, block)


def _attach(o, origin, extent, block, **kw):
    return (o.coarse_trace(HYD, HYD_PAIRS, block=block, origin=origin, extent=extent, **kw),
            o.coarse_trace(BAR, block=block, origin=origin, extent=extent, source="hydrovsbar", **kw))


# ---- 1. against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cb.CASES, ids=cb.case_id)
def test_lone_record_equals_the_twin(pkg, case):
    n, origin, extent, block = case
    lbm = _mixture(pkg, n)
    lbm.LBM_timestep(5)
    traces = _attach(lbm, origin, extent, block, capacity=1)
    for tr, nq in zip(traces, (5, 1)):
        assert tr.geometry() == cb.geometry(extent, block, nq)
        tr.sample()
    want = _want(pkg, lbm, origin, extent, block)
    sites = block[0] * block[1] * block[2]
    for tr, w in zip(traces, want):
        steps, sums = tr.read()
        assert steps.tolist() == [[5]] and steps.dtype == np.int64 and sums.shape == (1, 1) + w.shape
        assert np.array_equal(sums[0, 0], w), (case, np.abs(sums[0, 0] - w).max())
        assert np.ptp(sums[0, 0, 0]) > 0                   # no uniform field
        assert np.array_equal(tr.means()[0, 0], sums[0, 0] / float(sites))
    assert traces[0].names == HYD and traces[0].sum_names == HYD + ["rho*phi", "ufx*ufx"] and traces[1].names == BAR
    if block == (1, 1, 1):                                 # the window itself, bit for bit
        hyd = lbm.LBM_hydrovars()[_index(pkg, HYD)]
        z0, z1 = origin[2], origin[2] + extent[2]
        assert np.array_equal(traces[0].read()[1][0, 0, :3], hyd[:, z0:z1])
    var = traces[0].block_variance(1)                      # <ufx ufx> - <ufx>^2 within every block
    mean = want[0][2] / sites
    assert np.array_equal(var[0, 0], want[0][4] / sites - mean * mean)
    lbm.close()


def test_eight_variables_and_sixteen_pairs(pkg):
    n, origin, extent, block = SEAM
    lbm = _mixture(pkg, n)
    lbm.LBM_timestep(5)
    variables = [0, 1, 2, 3, 4, 9, 12, 21]                 # rho phi ufx ufy ufz afx agx ugbarx
    pairs = [(k % 8, (3 * k) % 8) for k in range(16)]
    tr = lbm.coarse_trace(variables, pairs, block=block, origin=origin, extent=extent, capacity=1)
    assert tr.geometry() == cb.geometry(extent, block, 24)
    tr.sample()
    want = pkg.analysis.coarse_fields(lbm.LBM_hydrovars()[variables], pairs, origin, extent, block)
    got = tr.read()[1][0, 0]
    assert got.shape == (24, 2, 2, 2) and np.array_equal(got, want), np.abs(got - want).max()
    lbm.close()


def test_sum_of_the_blocks_within_the_bound_of_a_recursive_sum(pkg):
    """rho over the full (8, 8, 8) box at block (2, 2, 2): the blocks added up against math.fsum of the field, within
    nsites 2^-53 fsum(|field|), the standard bound of a recursive sum of nsites terms in any order."""
    n = (8, 8, 8)
    lbm = _mixture(pkg, n)
    lbm.LBM_timestep(5)
    tr = lbm.coarse_trace(["rho"], block=(2, 2, 2), capacity=1)
    tr.sample()
    blocks = tr.read()[1][0, 0, 0]
    rho = lbm.LBM_hydrovars()[0]
    total = 0.0
    for v in blocks.ravel().tolist():
        total += v
    exact, bound = math.fsum(rho.ravel().tolist()), 512 * 2.0 ** -53 * math.fsum(np.abs(rho).ravel().tolist())
    print("sum of the blocks %.17g, fsum %.17g, difference %.3e, bound %.3e" % (total, exact, abs(total - exact), bound))
    assert blocks.shape == (4, 4, 4) and abs(total - exact) <= bound
    lbm.close()


# ---- 2. batches ------------------------------------------------------------------------------------------------------------
def test_batch_record_equals_the_twin_the_lone_lattice_and_a_smaller_batch(pkg):
    n, origin, extent, block = SEAM
    batch = _batch(pkg, n)
    batch.LBM_timestep(5)
    traces = _attach(batch, origin, extent, block, capacity=1)
    for tr, nq in zip(traces, (5, 1)):
        assert tr.geometry() == cb.geometry(extent, block, nq, 3)
        tr.sample()
    got = [tr.read() for tr in traces]
    for r, v in enumerate(batch.replicas):
        for (steps, sums), w in zip(got, _want(pkg, v, origin, extent, block)):
            assert steps.tolist() == [[5, 5, 5]] and sums.shape == (1, 3) + w.shape
            assert np.array_equal(sums[0, r], w), (r, np.abs(sums[0, r] - w).max())
    assert not np.array_equal(got[0][1][0, 0], got[0][1][0, 1])            # the replicas differ
    batch.close()
    for r, p in enumerate(_params()):                      # every replica run alone
        lbm = _mixture(pkg, n, **p)
        lbm.LBM_timestep(5)
        for tr, (steps, sums) in zip(_attach(lbm, origin, extent, block, capacity=1), got):
            tr.sample()
            assert np.array_equal(tr.read()[1][0, 0], sums[0, r]), r
        lbm.close()
    pair = _batch(pkg, n, params=_params()[1:])            # replicas 1 and 2 inside a batch of 2
    pair.LBM_timestep(5)
    for tr, (steps, sums) in zip(_attach(pair, origin, extent, block, capacity=1), got):
        tr.sample()
        assert np.array_equal(tr.read()[1][0], sums[0, 1:])
    pair.close()


# ---- 3. cadence and lifecycle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n, origin, extent, block = SEAM
    o = _mixture(pkg, n) if owner == "lone" else _batch(pkg, n)
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: max(v.steps_done for v in o.replicas))
    other = o.trace(every=1, capacity=16)
    tr = o.coarse_trace(["rho", "phi"], [("rho", "phi")], block=block, origin=origin, extent=extent, every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="coarse trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    tr.sample()                                                          # twice on the same state: equal slots
    steps, sums = tr.read()
    assert tr.count == 2 and steps[:, 0].tolist() == [0, 0] and done() == 0 and np.array_equal(sums[0], sums[1])
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    steps, sums = tr.read()
    with pytest.raises(pkg.BflbmError, match="coarse trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="coarse trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, sums2 = tr.read()
    assert np.array_equal(sums, sums2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    assert not np.array_equal(sums[0], sums[1]) and not np.array_equal(sums[1], sums[2])
    w_steps, w_sums = tr.read(first=1, count=2)                          # a window of the record
    assert np.array_equal(w_sums, sums[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[0][0, 0] == 7
    # the owner goes first: the trace stays readable with the same bits, refuses a sample, closes twice
    steps, sums = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, sums2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(sums, sums2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_creation_refusals(pkg):
    n = (10, 6, 13)
    lbm, batch = _mixture(pkg, n), _batch(pkg, n)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_coarse_create.*replica of a batch.*use bflbm_batch_coarse_create"):
        batch.replicas[0].coarse_trace(["rho"])
    for owner, call in ((lbm, "bflbm_coarse_create"), (batch, "bflbm_batch_coarse_create")):
        nrep = 3 if owner is batch else 1
        for pattern, variables, pairs, kw in (("variable index 22 outside hydrovs", [0, 22], [], {}),
                                              ("variable index 9 outside hydrovsbar", [9], [], dict(source="hydrovsbar")),
                                              ("variable index 3 given twice", [3, 1, 3], [], {}),
                                              ("1..8 variables", list(range(9)), [], {}),
                                              ("0..16 pairs", [0], [(0, 0)] * 17, {}),
                                              ("pair 1: slot 2 outside the 2 variables", [0, 1], [(0, 1), (2, 0)], {}),
                                              (r"origin\[x\] = 10 outside 0..9", [0], [], dict(origin=(10, 0, 0), extent=(1, 1, 1))),
                                              (r"origin\[z\] = -1 outside 0..12", [0], [], dict(origin=(0, 0, -1), extent=(1, 1, 1))),
                                              (r"extent\[y\] = 7 outside 1..6", [0], [], dict(extent=(10, 7, 13))),
                                              (r"extent\[x\] = 0 outside 1..10", [0], [], dict(extent=(0, 6, 13))),
                                              (r"block\[z\] must be >= 1 \(got 0\)", [0], [], dict(block=(1, 1, 0))),
                                              (r"block\[x\] = 3 does not divide the extent 10", [0], [], dict(block=(3, 1, 1))),
                                              (r"block\[y\] = 4 does not divide the extent 5", [0], [], dict(origin=(0, 1, 0), block=(1, 4, 1))),
                                              ("every must be >= 1", [0], [], dict(every=0)),
                                              ("capacity must be >= 1", [0], [], dict(capacity=0)),
                                              ("exceeds 1 TB", [0], [], dict(capacity=(1 << 37) // (780 * nrep) + 1))):
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                owner.coarse_trace(variables, pairs, **kw)
            assert call in str(e.value), (call, str(e.value))
        assert not getattr(owner, "_dependents", [])       # nothing was attached
    for bad in (lambda: lbm.coarse_trace(["no_such_variable"]), lambda: lbm.coarse_trace(["rho"], [("phi", "rho")]),
                lambda: lbm.coarse_trace(["rho"], source="noise"), lambda: lbm.coarse_trace(["rho"], block=(1, 1)),
                lambda: lbm.coarse_trace(["rho"], origin=3)):
        with pytest.raises(ValueError):
            bad()
    tr = lbm.coarse_trace(["rho"], [("rho", "rho")], capacity=2)
    with pytest.raises(ValueError):
        tr.block_variance(1)
    tr.close()
    assert not hasattr(pkg.RingLBM, "coarse_trace")
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_coarse_create inside an open step"):
        lbm.coarse_trace(["rho"])
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.coarse_trace(["rho"], capacity=2)
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
    with pytest.raises(pkg.BflbmError, match=r"bflbm_coarse_create.*nranks > 1"):
        slab.coarse_trace(["rho"])
    slab.close()


# ---- 4. a recorder changes nothing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,schedule", [((12, 10, 14), "fused"), ((64, 8, 12), "handover")])
def test_a_coarse_trace_changes_nothing(pkg, n, schedule):
    a, b = _mixture(pkg, n, schedule), _mixture(pkg, n, schedule)
    assert a.resolved_schedule() == schedule and b.resolved_schedule() == schedule
    traces = [a.coarse_trace(HYD, HYD_PAIRS, block=(2, 2, 2), every=1, capacity=13),
              a.coarse_trace(BAR, block=(1, 1, 1), origin=(n[0] - 2, 3, 5), extent=(4, 5, 1), source="hydrovsbar", every=1, capacity=13)]
    a.LBM_timestep(12); b.LBM_timestep(12)
    assert a.steps_done == b.steps_done == 12 and all(tr.count == 12 for tr in traces)
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    a.LBM_timestep(1); b.LBM_timestep(1)                   # the step after the last sample
    for u, v in zip(a.populations(), b.populations()):
        assert np.array_equal(u, v)
    steps, sums = traces[0].read()
    assert steps[:, 0].tolist() == list(range(1, 14)) and np.isfinite(sums).all() and not np.array_equal(sums[0], sums[12])
    a.close(); b.close()


# ---- 5. coexistence ------------------------------------------------------------------------------------------------------------
def test_coarse_histogram_and_profile_traces_on_one_owner(pkg):
    """The three read the same observation out of the scratch state buffer, one after the other: each record equals the
    record of the kind attached alone."""
    n = (12, 10, 14)
    kinds = {"coarse": lambda o: o.coarse_trace(HYD, HYD_PAIRS, block=(3, 5, 2), origin=(7, 0, 9), extent=(12, 10, 8), every=1, capacity=4),
             "hist": lambda o: o.histogram_trace({"phi": (0.9, 1.1, 16), "ufy": (-1e-2, 1e-2, 8)}, [("phi", "ufy")], every=1, capacity=4),
             "profile": lambda o: o.profile_trace(["rho", "agx"], [("rho", "agx")], axis="x", every=1, capacity=4)}

    def records(names):
        lbm = _mixture(pkg, n)
        traces = {k: kinds[k](lbm) for k in names}
        lbm.LBM_timestep(4)
        out = {k: [np.array(v) for v in tr.read()] for k, tr in traces.items()}
        lbm.close()
        return out
    together = records(["coarse", "hist", "profile"])
    swapped = records(["profile", "hist", "coarse"])
    for k in kinds:
        alone = records([k])[k]
        for rec in (together[k], swapped[k]):
            assert all(np.array_equal(u, v) for u, v in zip(rec, alone)), k
    steps, sums = together["coarse"]
    assert steps[:, 0].tolist() == [1, 2, 3, 4] and sums.shape == (4, 1, 5, 4, 2, 4) and not np.array_equal(sums[0], sums[3])
