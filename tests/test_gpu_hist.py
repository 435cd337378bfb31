"""GPU: histogram traces (HistogramTrace, bflbm_hist_*): the counts of the sites of chosen variables over fixed bins and
of pairs of them over two binnings, recorded on the device as 64-bit integers.

The binning rule and the layout of a sample are in include/bflbm.h ("Histogram traces"); analysis.field_histograms
restates the rule in numpy and tests/test_hist_abi.py holds it to a site-by-site loop.  Here the device record is compared
with field_histograms of the fields the same lattice hands out, integer for integer: lone lattices and all three sources,
replicas of a batch, rings of z-slabs.  Every record's blocks sum to the site count."""
import ctypes
import math

import numpy as np
import pytest

import hist_counts as hc

pytestmark = pytest.mark.gpu

# source -> ({variable: bins}, pairs); hydrovsbar not in ascending order
CASES = {"hydrovs": ({"rho": 64, "phi": 33, "ufx": 100, "agz": 7}, [("rho", "phi"), ("ufx", "rho")]),
         "hydrovsbar": ({"phi": 16, "rho": 5, "ufy": 1}, [("phi", "rho")]),
         "noise": ({"fa1": 50, "ga4": 9}, [("fa1", "ga4")])}
BOXES = [(7, 9, 5),          # 315 sites: an odd count, the scalar tail, volumes that are not 16-byte aligned
         (64, 32, 3),        # three full tiles of 2048 sites
         (66, 32, 3),        # a last, short tile
         (130, 3, 2)]        # 780 sites: less than a tile
BIG = (128, 64, 129)         # 516 tiles on 512 workgroups: four workgroups take a second tile
STATES = ["quiet", "stripe", "noisy", "planted"]


def _schedule(n):
    return "fused" if min(n) >= 5 else "two_pass"


def _lattice(pkg, n, state, **params):
    """quiet: a zero-noise mixture, every site in one bin; stripe: runs of equal bins; noisy: a mixture at kBT = 1e-5
    after 5 steps, scattered bins; planted: the noisy state uploaded again with NaN and huge populations at four sites."""
    p = dict(kBT=0.0 if state in ("quiet", "stripe") else 1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0, seed=77)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=_schedule(n))
    if state == "stripe":
        lbm.LBM_init_stripe(0.5)
        lbm.LBM_timestep(2)
    else:
        lbm.LBM_init_mixture()
        lbm.LBM_timestep(0 if state == "quiet" else 5)
    if state == "planted":
        f, g = lbm.populations()
        flat_f, flat_g = f.reshape(f.shape[0], -1), g.reshape(g.shape[0], -1)
        sites = flat_f.shape[1]
        flat_f[:, sites // 3] = np.nan
        flat_g[3, sites // 2] = np.nan
        flat_f[0, sites - 1] = 1e200
        flat_g[0, 0] = -1e200
        lbm.LBM_init(f, g)
    return lbm


def _components(pkg, source, names):
    if source == "noise":
        return [(19 if v[0] == "g" else 0) + int(v[2:]) for v in names]
    all_names = pkg.plotfile.variable_names(9 if source == "hydrovsbar" else 22)
    return [all_names.index(v) for v in names]


def _fields(pkg, lat, source, names):
    """The chosen variables of the resident state through the full-field getters: [nvars][nz][ny][nx]."""
    if source == "noise":
        full = np.concatenate(lat.thermal_noise())
    else:
        full = lat.LBM_hydrovars() if source == "hydrovs" else lat.LBM_hydrovars_density()
    return full[_components(pkg, source, names)].copy()


def _range(x, nbins):
    """A range that leaves some of the finite values of x on either side: between the 10 % and 90 % quantiles; around the
    value where those coincide (a uniform field); (-1, 1) where nothing usable is there."""
    finite = x[np.isfinite(x)]
    if finite.size:
        a, b = (float(v) for v in np.quantile(finite, [0.1, 0.9]))
        if not b > a:
            a, b = a - 1.0, a + 1.0
        with np.errstate(over="ignore", divide="ignore"):
            scale = nbins / (b - a)
        if math.isfinite(scale) and scale > 0:
            return a, b
    return -1.0, 1.0


def _ranges(fields, bins):
    return {v: _range(fields[k], nb) + (nb,) for k, (v, nb) in enumerate(bins.items())}


def _twin(pkg, fields, ranges, pairs):
    names = list(ranges)
    lo, hi, nb = zip(*ranges.values())
    return pkg.analysis.field_histograms(fields, lo, hi, nb, [(names.index(a), names.index(b)) for a, b in pairs])


def _check_blocks(tr, counts, n):
    """Every variable block and every pair block of every sample sums to nx ny nz."""
    sums = hc.block_sums(counts, tr.geometry()[1])
    assert (sums == n[0] * n[1] * n[2]).all(), sums


# ---- 1. a lone lattice against the twin, every source -----------------------------------------------------------------------
@pytest.mark.parametrize("n,state", [(n, s) for n in BOXES for s in STATES] + [(BIG, "noisy")])
def test_lone_record_equals_the_twin(pkg, n, state):
    lbm = _lattice(pkg, n, state)
    steps_done = lbm.steps_done
    seen = {}
    for source, (bins, pairs) in CASES.items():
        names = list(bins)
        fields = _fields(pkg, lbm, source, names)
        ranges = _ranges(fields, bins)
        tr = lbm.histogram_trace(ranges, pairs, source=source, capacity=1)
        geo = tr.geometry()
        assert geo == hc.geometry(n, list(bins.values()), [(names.index(a), names.index(b)) for a, b in pairs])
        if n == BIG:
            assert geo[3] == 512 and (n[0] * n[1] * n[2] + geo[2] - 1) // geo[2] == 516      # a workgroup takes a second tile
        tr.sample()
        steps, counts = tr.read()
        want = _twin(pkg, fields, ranges, pairs)              # the getters leave the resident state as it is
        assert counts.shape == (1, 1, geo[0]) and counts.dtype == np.int64 and steps.tolist() == [[steps_done]]
        differ = np.flatnonzero(counts[0, 0] != want)
        assert differ.size == 0, (n, state, source, differ[:8], counts[0, 0][differ[:8]], want[differ[:8]])
        _check_blocks(tr, counts, n)
        assert tr.names == names and np.array_equal(tr.hist(names[0])[0, 0], want[:bins[names[0]]])
        seen[source] = (counts[0, 0], tr, bins)
    c, tr, bins = seen["hydrovs"]
    if state == "quiet":                                   # the contention path: every site in one bin, one cell
        assert tr.hist("rho").max() == n[0] * n[1] * n[2] and tr.joint(("rho", "phi"))[0].max() == n[0] * n[1] * n[2]
    if state == "stripe":                                  # runs: more than one bin, far fewer than sites
        assert 1 < np.count_nonzero(tr.hist("rho")) + np.count_nonzero(tr.outliers("rho")) <= bins["rho"] + 2
    if state == "noisy":
        assert np.count_nonzero(tr.hist("ufx")) > 50 and tr.outliers("ufx")[0, 0, :2].min() > 0 and tr.outliers("ufx")[0, 0, 2] == 0
    if state == "planted":
        assert tr.outliers("rho")[0, 0, 2] >= 1 and tr.outliers("agz")[0, 0, 2] >= 1 and tr.joint(0)[1][0, 0] >= 1
    lbm.close()
    for _, tr, _ in seen.values():
        tr.close()


def test_edges_taken_from_site_values_and_the_large_lds_class(pkg):
    """lo and hi are two site values of the downloaded field, so both edges are hit exactly: the site at lo counts in
    bin 0, the site at hi where (hi - lo) * scale falls.  4096 bins of ufx and a 100 x 100 pair give C = 14306: the 64 KiB instantiation."""
    n = (66, 32, 3)
    lbm = _lattice(pkg, n, "noisy")
    names = ["ufx", "rho", "phi"]
    fields = _fields(pkg, lbm, "hydrovs", names)
    ranges = {}
    for k, (v, nb) in enumerate(zip(names, (4096, 100, 100))):
        values = np.unique(fields[k])
        ranges[v] = (float(values[len(values) // 10]), float(values[-len(values) // 10]), nb)
    pairs = [("rho", "phi")]
    tr = lbm.histogram_trace(ranges, pairs, capacity=1)
    assert tr.geometry() == hc.geometry(n, [4096, 100, 100], [(1, 2)]) and tr.geometry()[0] == 14306 and tr.geometry()[4] == 16384
    tr.sample()
    counts = tr.read()[1]
    want = _twin(pkg, fields, ranges, pairs)
    assert np.array_equal(counts[0, 0], want)
    _check_blocks(tr, counts, n)
    for k, v in enumerate(names):
        lo, hi, nb = ranges[v]
        assert tr.hist(v)[0, 0, 0] >= np.count_nonzero(fields[k] == lo) >= 1          # t = 0 exactly
        assert tr.outliers(v)[0, 0, 0] == np.count_nonzero(fields[k] < lo) >= 1
        assert np.count_nonzero(fields[k] == hi) >= 1 and tr.outliers(v)[0, 0, 1] >= 1    # where hi itself goes is the rule's: the twin says
        assert tr.edges(v).shape == (nb + 1,) and tr.edges(v)[0] == lo and tr.edges(v)[-1] == hi
        pdf = tr.pdf(v)[0, 0]
        assert abs(pdf.sum() * (hi - lo) / nb - 1.0) < 1e-12
    cells, outside = tr.joint(("rho", "phi"))
    assert cells.shape == (1, 1, 100, 100) and cells.sum() + outside[0, 0] == n[0] * n[1] * n[2]
    lbm.close(); tr.close()


# ---- 2. a batch ---------------------------------------------------------------------------------------------------------------
def _batch_params():
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


@pytest.mark.parametrize("source", ["hydrovs", "hydrovsbar"])
def test_batch_replicas_equal_the_twin_and_the_lattice_run_alone(pkg, source):
    n = (13, 10, 6)
    bins, pairs = CASES[source]
    names = list(bins)
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    batch.LBM_timestep(3)
    ranges = _ranges(_fields(pkg, batch.replicas[0], source, names), bins)      # one binning for all replicas
    tr = batch.histogram_trace(ranges, pairs, source=source, every=2, capacity=4)
    assert tr.geometry() == hc.geometry(n, list(bins.values()), [(names.index(a), names.index(b)) for a, b in pairs], nrep=3)
    tr.sample()
    steps, counts = tr.read()
    assert steps.tolist() == [[3, 1003, 3]] and counts.shape[:2] == (1, 3)
    for r, v in enumerate(batch.replicas):
        assert np.array_equal(counts[0, r], _twin(pkg, _fields(pkg, v, source, names), ranges, pairs)), (source, r)
    assert not np.array_equal(counts[0, 0], counts[0, 1]) and not np.array_equal(counts[0, 0], counts[0, 2])
    batch.LBM_timestep(4)                                  # samples after the batch steps 2 and 4
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == [3, 5, 7]
    _check_blocks(tr, counts, n)
    batch.close()
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        if r == 1:
            lone.set_steps_done(1000)
        lone.LBM_timestep(3)
        alone = lone.histogram_trace(ranges, pairs, source=source, every=2, capacity=4)
        alone.sample()
        lone.LBM_timestep(4)
        a_steps, a_counts = alone.read()
        assert np.array_equal(a_steps[:, 0], steps[:, r]) and np.array_equal(a_counts[:, 0], counts[:, r]), (source, r)
        lone.close(); alone.close()
    assert np.array_equal(tr.read()[1], counts)            # detached, still readable
    tr.close()


# ---- 3. a ring of z-slabs -----------------------------------------------------------------------------------------------------
def test_ring_record_equals_the_lone_record(pkg):
    n = (16, 8, 12)
    par = dict(alpha0=1.0, kBT=1e-5, tau_f=1.0, tau_g=1.0, seed=7)
    probe = pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule="fused")
    probe.LBM_init_mixture()
    probe.LBM_timestep(3)
    ranges = {s: _ranges(_fields(pkg, probe, s, list(CASES[s][0])), CASES[s][0]) for s in ("hydrovs", "noise")}
    probe.close()
    records = {}
    for nslabs in (0, 1, 2, 3):                            # 0: the lone lattice
        if nslabs == 0:
            o = pkg.BinaryLBM(*n, params=pkg.default_params(**par), schedule="fused")
        else:
            o = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**par), schedule="fused")
        o.LBM_init_mixture()
        hyd = o.histogram_trace(ranges["hydrovs"], CASES["hydrovs"][1], every=2, capacity=4)
        noise = o.histogram_trace(ranges["noise"], CASES["noise"][1], source="noise", every=3, capacity=2)
        hyd.sample()
        o.LBM_timestep(6)
        records[nslabs] = hyd.read() + noise.read()
        _check_blocks(hyd, records[nslabs][1], n)
        _check_blocks(noise, records[nslabs][3], n)
        if nslabs in (2, 3):                               # the last sample against the gathered fields
            want = _twin(pkg, o.LBM_hydrovars()[_components(pkg, "hydrovs", list(ranges["hydrovs"]))], ranges["hydrovs"], CASES["hydrovs"][1])
            assert np.array_equal(records[nslabs][1][-1, 0], want), nslabs
        # which creation call served the owner: a ring of one slab gets the lone recorder
        with pytest.raises(pkg.BflbmError) as e:
            o.histogram_trace({"rho": (0.0, 1.0, 4)}, every=0)
        assert ("bflbm_ring_hist_create" if nslabs > 1 else "bflbm_hist_create") in str(e.value)
        o.close()
        hyd.close(); noise.close()
    lone = records[0]
    assert lone[0][:, 0].tolist() == [0, 2, 4, 6] and lone[2][:, 0].tolist() == [3, 6]
    assert not np.array_equal(lone[1][1], lone[1][2]) and np.count_nonzero(lone[3][0, 0]) > 20
    for nslabs in (1, 2, 3):
        for a, b in zip(records[nslabs], lone):
            assert np.array_equal(a, b), nslabs


# ---- 4. independence of what else is attached, of `every` and of the capacity ---------------------------------------------------
def test_record_does_not_depend_on_the_other_recorders_every_or_capacity(pkg):
    n = (13, 10, 6)
    bins, pairs = CASES["hydrovs"]
    modes = np.array([(1, 0, 0), (0, 1, 1)])
    probe = _lattice(pkg, n, "noisy")
    ranges = _ranges(_fields(pkg, probe, "hydrovs", list(bins)), bins)
    probe.close()
    records = {}
    for order in ("alone", "after the others"):
        lbm = _lattice(pkg, n, "noisy")
        others = []
        if order != "alone":
            others = [lbm.field_stats(["rho", "phi"], [("rho", "phi")], every=1), lbm.mode_trace(["rho", "ubx"], modes, every=1, capacity=8),
                      lbm.spectrum_trace(["rho", "phi"], every=1, capacity=8), lbm.profile_trace(["rho", "afz"], [("rho", "afz")], axis="y", every=1, capacity=8),
                      lbm.radial_trace(["rho", "phi"], [("rho", "phi")], centre=(6.0, 5.0, 3.0), every=1, capacity=8)]
        tr = lbm.histogram_trace(ranges, pairs, every=2 if order == "alone" else 1, capacity=3 if order == "alone" else 16)
        lbm.LBM_timestep(6)
        assert all(r.count == 6 for r in others)
        records[order] = tr.read()
        lbm.close(); tr.close()
    steps, counts = records["alone"]
    assert steps[:, 0].tolist() == [7, 9, 11] and not np.array_equal(counts[0], counts[2])
    steps2, counts2 = records["after the others"]
    assert steps2[:, 0].tolist() == [6, 7, 8, 9, 10, 11]
    assert np.array_equal(counts2[1::2], counts)


# ---- 5. automatic sampling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("owner", ["lone", "batch"])
def test_overflow_is_refused_whole_and_reset_restarts(pkg, owner):
    n = (9, 7, 5)
    if owner == "lone":
        o = _lattice(pkg, n, "noisy")
        o.set_steps_done(0)
    else:
        o = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
        for v in o.replicas:
            v.LBM_init_mixture()
    done = (lambda: o.steps_done) if owner == "lone" else (lambda: o.replicas[0].steps_done)
    other = o.trace(every=1, capacity=16)
    tr = o.histogram_trace({"rho": (0.4, 0.6, 32), "phi": (0.4, 0.6, 8)}, [("rho", "phi")], every=2, capacity=3)
    with pytest.raises(pkg.BflbmError, match="histogram trace full"):
        o.LBM_timestep(8)
    assert done() == 0 and tr.count == 0 and other.count == 0            # refused whole: nothing stepped, nothing recorded
    tr.sample()                                                          # frame 0: a hand sample
    assert tr.count == 1 and tr.read()[0][0, 0] == 0 and done() == 0
    tr.reset()
    o.LBM_timestep(3)                                                    # a sample after step 2
    tr.sample()                                                          # by hand after step 3: the every-count does not move
    o.LBM_timestep(2)                                                    # steps 4 and 5: a sample after step 4
    assert done() == 5 and tr.count == 3 and other.count == 5
    state = [u.copy() for u in o.populations()]
    steps, counts = tr.read()
    with pytest.raises(pkg.BflbmError, match="histogram trace full"):
        o.LBM_timestep(1)                                                # step 6 is due a sample
    with pytest.raises(pkg.BflbmError, match="histogram trace full"):
        tr.sample()
    assert done() == 5 and tr.count == 3 and other.count == 5
    assert all(np.array_equal(u, v) for u, v in zip(state, o.populations()))
    steps2, counts2 = tr.read()
    assert np.array_equal(counts, counts2) and np.array_equal(steps, steps2)
    assert steps[:, 0].tolist() == [2, 3, 4]
    _check_blocks(tr, counts, n)
    w_steps, w_counts = tr.read(first=1, count=2)                         # a window of the record
    assert np.array_equal(w_counts, counts[1:]) and np.array_equal(w_steps, steps[1:])
    tr.reset()
    assert tr.count == 0 and tr.read()[1].shape[0] == 0
    o.LBM_timestep(2)                                                    # the every-count restarted: steps 6, 7 sample at 7
    assert tr.count == 1 and tr.read()[0][0, 0] == 7
    # the owner goes first: the trace stays readable with the same integers, refuses a sample, closes twice
    steps, counts = tr.read()
    geo = tr.geometry()
    o.close()
    assert tr._h is not None
    steps2, counts2 = tr.read()
    assert np.array_equal(steps, steps2) and np.array_equal(counts, counts2) and tr.geometry() == geo
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        tr.sample()
    tr.close(); tr.close()
    assert tr._h is None


def test_histogram_trace_outlives_its_owner_through_the_abi(pkg):
    lib, check = pkg._lib.load(), pkg._lib.check
    lbm = _lattice(pkg, (9, 7, 5), "noisy")
    lbm.set_steps_done(0)
    t = ctypes.c_void_p()
    va, nb = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 2)(6, 3)
    lo, hi = (ctypes.c_double * 2)(0.45, 0.45), (ctypes.c_double * 2)(0.55, 0.55)
    pa, pb = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0)
    check(lib.bflbm_hist_create(lbm._h, 1, 2, va, lo, hi, nb, 1, pa, pb, 1, 4, ctypes.byref(t)))
    lbm.LBM_timestep(3)
    C = 9 + 6 + 19
    as_ll = ctypes.POINTER(ctypes.c_longlong)

    def read(first, count):
        counts, steps = np.empty((count, 1, C), dtype=np.int64), np.empty((count, 1), dtype=np.int64)
        check(lib.bflbm_hist_read(t, first, count, counts.ctypes.data_as(as_ll), steps.ctypes.data_as(as_ll)))
        return counts, steps
    counts0, steps0 = read(0, 3)
    assert steps0[:, 0].tolist() == [1, 2, 3] and (hc.block_sums(counts0, [(0, 9), (9, 6), (15, 19)]) == 315).all()
    handle = lbm._h
    lbm._h = None                                          # the wrapper lets go; the context is destroyed below
    check(lib.bflbm_destroy(handle))
    counts1, steps1 = read(0, 3)
    assert np.array_equal(steps0, steps1) and np.array_equal(counts0, counts1)
    assert np.array_equal(read(2, 1)[0][0], counts0[2])    # a window
    assert lib.bflbm_hist_read(t, 2, 2, counts0.ctypes.data_as(as_ll), None) != 0
    assert lib.bflbm_hist_sample(t) != 0 and "destroyed" in lib.bflbm_last_error().decode()
    check(lib.bflbm_hist_destroy(t))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_creation_refusals(pkg):
    n = (8, 8, 8)
    lbm = _lattice(pkg, n, "noisy")
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    ring = pkg.RingLBM(*n, nslabs=2, devices=(0,), params=pkg.default_params(kBT=1e-5))
    ring.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match=r"bflbm_hist_create.*replica of a batch.*use bflbm_batch_hist_create"):
        batch.replicas[0].histogram_trace({"rho": (0, 1, 4)})
    with pytest.raises(pkg.BflbmError, match=r"bflbm_batch_hist_create.*no noise form"):
        batch.histogram_trace({"fa1": (-1, 1, 4)}, source="noise")
    r4 = (0.0, 1.0, 4)
    for owner, call in ((lbm, "bflbm_hist_create"), (batch, "bflbm_batch_hist_create"), (ring, "bflbm_ring_hist_create")):
        nrep = 3 if owner is batch else 1
        for pattern, ranges, pairs, kw in (("variable index 22 outside hydrovs", {0: r4, 22: r4}, [], {}),
                                           ("variable index -1 outside hydrovs", {-1: r4}, [], {}),
                                           ("variable index 9 outside hydrovsbar", {9: r4}, [], dict(source="hydrovsbar")),
                                           ("variable index 3 given twice", [(3, 0, 1, 4), (1, 0, 1, 4), (3, 0, 1, 4)], [], {}),
                                           ("1..8 variables", {k: r4 for k in range(9)}, [], {}),
                                           ("1..8 variables", {}, [], {}),
                                           ("0..4 pairs", {0: r4, 1: r4}, [(0, 1)] * 5, {}),
                                           ("pair 1: slot 2 outside the 2 variables", {0: r4, 1: r4}, [(0, 1), (2, 0)], {}),
                                           ("pair 0: slot -1 outside the 1 variables", {0: r4}, [(0, -1)], {}),
                                           ("pair 0: slot 1 with itself", {0: r4, 1: r4}, [(1, 1)], {}),
                                           ("slot 1: the range needs finite lo < hi", {0: r4, 1: (np.nan, 1.0, 4)}, [], {}),
                                           ("slot 0: the range needs finite lo < hi", {0: (0.0, np.inf, 4)}, [], {}),
                                           ("slot 0: the range needs finite lo < hi", {0: (-np.inf, 0.0, 4)}, [], {}),
                                           ("slot 0: the range needs finite lo < hi", {0: (1.0, 1.0, 4)}, [], {}),
                                           ("slot 0: the range needs finite lo < hi", {0: (1.0, 0.0, 4)}, [], {}),
                                           ("slot 0: the scale .* is not finite and positive", {0: (-1.7e308, 1.7e308, 4)}, [], {}),
                                           ("slot 0: the scale .* is not finite and positive", {0: (0.0, 5e-324, 4)}, [], {}),
                                           ("slot 1: 1..4096 bins", {0: r4, 1: (0.0, 1.0, 0)}, [], {}),
                                           ("slot 0: 1..4096 bins", {0: (0.0, 1.0, 4097)}, [], {}),
                                           ("16390 counters per replica exceed 16384", {0: (0.0, 1.0, 127), 1: (0.0, 1.0, 127)}, [(0, 1)], {}),
                                           ("source must be 0", {0: r4}, [], dict(source=3)),
                                           ("every must be >= 1", {0: r4}, [], dict(every=0)),
                                           ("capacity must be >= 1", {0: r4}, [], dict(capacity=0)),
                                           ("exceeds 1 TB", {0: r4}, [], dict(capacity=(1 << 37) // (7 * nrep) + 1))):
            direct = {k: kw.pop(k) for k in ("source",) if k in kw and not isinstance(kw[k], str)}
            with pytest.raises(pkg.BflbmError, match=pattern) as e:
                if direct:                                 # past the wrapper's own checks: through the ABI
                    h = ctypes.c_void_p()
                    va, nb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(4)
                    lo, hi = (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(1.0)
                    pkg._lib.check(getattr(pkg._lib.load(), call)(owner._h, direct["source"], 1, va, lo, hi, nb, 0, None, None, 1, 4, ctypes.byref(h)))
                else:
                    owner.histogram_trace(ranges, pairs, **kw)
            assert call in str(e.value), (call, str(e.value))
        # null range and bin arrays, through the ABI
        h = ctypes.c_void_p()
        va, nb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(4)
        lo, hi = (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(1.0)
        for args in ((None, hi, nb), (lo, None, nb), (lo, hi, None)):
            assert getattr(pkg._lib.load(), call)(owner._h, 0, 1, va, *args, 0, None, None, 1, 4, ctypes.byref(h)) != 0
            assert "null argument" in pkg._lib.load().bflbm_last_error().decode() and not h.value
        assert not getattr(owner, "_dependents", [])       # nothing was attached
        # the limits themselves: 8 variables, 4 pairs, C = 8 x 67 + 4 x 4097 = 16924 is too many, 8 x 35 + 4 x 1025 = 4380 fits
        full = owner.histogram_trace({k: (0.0, 1.0, 32) for k in range(8)}, [(k, k + 4) for k in range(4)], capacity=1)
        full.sample()
        assert full.geometry()[0] == 4380 and (hc.block_sums(full.read()[1], full.geometry()[1]) == 512).all()
        full.close()
    for bad in (lambda: lbm.histogram_trace({"no_such_variable": r4}), lambda: lbm.histogram_trace({"rho": r4}, [("phi", "rho")]),
                lambda: lbm.histogram_trace({"rho": (0.0, 1.0)}), lambda: lbm.histogram_trace({"rho": r4}, source="moments")):
        with pytest.raises(ValueError):
            bad()
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="bflbm_hist_create inside an open step"):
        lbm.histogram_trace({"rho": r4})
    lbm.step_interior(); lbm.step_finish()
    tr = lbm.histogram_trace({"rho": r4}, capacity=2)
    tr.sample()
    lbm.step_boundary()
    for call in (tr.sample, tr.read, tr.reset):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    assert tr.count == 2 and tr.read()[0][:, 0].tolist() == [6, 7]       # the split step samples in its finish
    lbm.close(); batch.close(); ring.close()
    # a slab of a decomposed lattice
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    with pytest.raises(pkg.BflbmError, match=r"bflbm_hist_create.*nranks > 1"):
        slab.histogram_trace({"rho": r4})
    slab.close()


# ---- 7. the velocity PDF of a fluctuating mixture -----------------------------------------------------------------------------------
def test_velocity_histogram_of_a_noisy_mixture(pkg):
    """32^3 mixture at kBT = 1e-5, tau = 1, alpha0 = 0: ufx over 64 bins in +-6 sqrt(kBT / <rho>), every 10 steps for 200
    steps.  Asserted: the mean from the bin centres of the last sample lies within half a bin width of the in-range mean of
    the final downloaded field (each value is within w / 2 of its bin centre).  Printed, not asserted (nobody had measured
    them, so no tolerance was fixed in advance): the ratio of the histogram variance to kBT / <rho> and the chi-square of
    the last sample against the Gaussian of the sample's own variance; DESIGN.md section 8 carries the figures."""
    n, kBT, nb = 32, 1e-5, 64
    lbm = pkg.BinaryLBM(n, n, n, params=pkg.default_params(kBT=kBT, alpha0=0.0, tau_f=1.0, tau_g=1.0, seed=11), schedule="fused")
    lbm.LBM_init_mixture()
    names = pkg.plotfile.variable_names(22)
    rho = float(lbm.LBM_hydrovars()[names.index("rho")].mean())
    sigma = math.sqrt(kBT / rho)
    lo, hi = -6.0 * sigma, 6.0 * sigma
    tr = lbm.histogram_trace({"ufx": (lo, hi, nb)}, every=10, capacity=20)
    lbm.LBM_timestep(200)
    steps, counts = tr.read()
    assert steps[:, 0].tolist() == list(range(10, 201, 10))
    _check_blocks(tr, counts, (n, n, n))
    ufx = lbm.LBM_hydrovars()[names.index("ufx")].reshape(-1)
    assert np.array_equal(counts[-1, 0], pkg.analysis.field_histograms(ufx[None], [lo], [hi], [nb]))
    t = (ufx - lo) * (nb / (hi - lo))
    inside = ufx[(t >= 0) & (t < nb)]
    h = tr.hist("ufx")
    mean, var = pkg.analysis.histogram_moments(h, lo, hi)
    w = (hi - lo) / nb
    # chi-square of the last sample against the Gaussian of its own variance, over the bins that expect 5 sites or more
    cdf = np.array([0.5 * (1.0 + math.erf((e - mean[-1, 0]) / math.sqrt(2.0 * var[-1, 0]))) for e in tr.edges("ufx")])
    expect = np.diff(cdf) * h[-1, 0].sum()
    keep = expect >= 5.0
    chi2 = float((((h[-1, 0] - expect) ** 2 / np.where(keep, expect, 1.0))[keep]).sum())
    print("ufx: <rho> = %.6f, histogram variance / (kBT / <rho>): last sample %.4f, mean over the samples after step 100 %.4f; "
          "|histogram mean - field mean| / w = %.4f; outliers of the last sample %s; chi-square %.1f over %d bins"
          % (rho, var[-1, 0] / (kBT / rho), var[10:, 0].mean() / (kBT / rho), abs(mean[-1, 0] - inside.mean()) / w,
             tr.outliers("ufx")[-1, 0].tolist(), chi2, int(keep.sum())))
    assert inside.size == h[-1, 0].sum() and abs(mean[-1, 0] - inside.mean()) <= 0.5 * w
    lbm.close(); tr.close()
