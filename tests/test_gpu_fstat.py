"""GPU: field statistics (FieldStats, bflbm_fstat_*): per-site running means and covariances over frames, accumulated
on the device for a lone lattice, a replica batch and a ring of z-slabs.

The definition is in include/bflbm.h ("Field statistics"); analysis.field_statistics restates it in numpy operation for
operation, so every comparison here is of equal doubles (observable_twins.same_doubles): the recorder's accumulators
against the restatement over the frames a twin run with the same seed downloads.  The runs use the bit-exact schedules
(fused; two_pass on the boxes with an extent below 5) and kBT = 1e-5, so that the frames differ."""
import ctypes
import filecmp
import os

import numpy as np
import pytest

from observable_twins import same_doubles

pytestmark = pytest.mark.gpu

MIXTURE = dict(kBT=1e-5, alpha0=1.0, tau_f=1.0, tau_g=1.0, seed=77)
BOXES = [(12, 10, 6),      # 720 sites: no multiple of 256 or 512
         (5, 3, 7),        # 105 sites: an odd count and an odd row, the scalar tail and volumes that are not 16-byte aligned
         (20, 4, 4)]       # nx > 16: the state's pitch differs from the dense row
# source -> (variables, pairs of slots)
CASES = {"hydrovs": (["rho", "phi", "rhot", "ufx"], [(0, 0), (0, 1), (3, 3)]),        # rhot: component 5, rho + phi
         "hydrovsbar": (["rho", "ufx", "ugz"], [(0, 0), (1, 2), (2, 2)]),
         "noise": (["fn1", "fn2", "fn3", "gn4"], [(0, 0), (1, 1), (2, 2), (3, 3)])}


def _schedule(n):
    return "fused" if min(n) >= 5 else "two_pass"


def _lone(pkg, n, **params):
    p = dict(MIXTURE)
    p.update(params)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=_schedule(n))
    lbm.LBM_init_mixture()
    return lbm


def _components(pkg, source, names):
    if source == "noise":
        return [(19 if v[0] == "g" else 0) + int(v[2:]) for v in names]
    all_names = pkg.plotfile.variable_names(9 if source == "hydrovsbar" else 22)
    return [5 if v == "rhot" else all_names.index(v) for v in names]


def _frame(pkg, lat, source, names):
    """The chosen variables of the resident state through the full-field getters: [nvars][nz][ny][nx]."""
    idx = _components(pkg, source, names)
    if source == "noise":
        full = np.concatenate(lat.thermal_noise())
    else:
        full = lat.LBM_hydrovars() if source == "hydrovs" else lat.LBM_hydrovars_density()
    return full[idx].copy()


def _read(fs, replica=0):
    nv, npairs = len(fs.variables), len(fs.pairs)
    return dict(sum=np.array([fs.sum(v, replica) for v in range(nv)]), first=np.array([fs.first(v, replica) for v in range(nv)]),
                mean=np.array([fs.mean(v, replica) for v in range(nv)]),
                prod=np.array([fs.prod(p, replica) for p in range(npairs)]).reshape((npairs,) + fs.shape),
                cov=np.array([fs.cov(p, replica) for p in range(npairs)]).reshape((npairs,) + fs.shape), N=fs.count)


def _same(got, want, what):
    assert got["N"] == want["N"], (what, got["N"], want["N"])
    for key in ("first", "sum", "prod", "mean", "cov"):
        assert same_doubles(got[key], want[key]), (what, key, np.abs(got[key] - want[key]).max())
    assert np.isfinite(got["sum"]).all() and np.isfinite(got["prod"]).all()


# ---- 1, 2. a lone lattice, every source, exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("source", sorted(CASES))
@pytest.mark.parametrize("n", BOXES)
def test_lone_accumulators_equal_the_restatement(pkg, n, source):
    names, pairs = CASES[source]
    rec, twin = _lone(pkg, n), _lone(pkg, n)
    fs = rec.field_stats(names, pairs, source=source, every=1)
    assert fs.variables == _components(pkg, source, names) and fs.pairs == pairs and fs.count == 0
    fs.sample()                                               # frame 0; the every-count does not move
    rec.LBM_timestep(5)
    frames = [_frame(pkg, twin, source, names)]
    for _ in range(5):
        twin.LBM_timestep(1)
        frames.append(_frame(pkg, twin, source, names))
    want = pkg.analysis.field_statistics(frames, pairs)
    got = _read(fs)
    _same(got, want, (n, source))
    assert np.abs(want["cov"]).max() > 0                      # the frames do differ
    assert same_doubles(fs.mean(names[1]), want["mean"][1]) and same_doubles(fs.cov((names[0], names[0])), want["cov"][0])
    assert same_doubles(fs.mean(0, replica=-1), (0.0 + want["sum"][0]) * (1.0 / 6.0))      # B = 1: the ensemble of one
    for a, b in zip(rec.populations(), twin.populations()):
        assert np.array_equal(a, b)
    assert rec.steps_done == twin.steps_done == 5
    fs.close(); rec.close(); twin.close()


# ---- 3. cadence and lifecycle ---------------------------------------------------------------------------------------------
def test_cadence_manual_sample_reset_and_detach(pkg):
    n = (12, 10, 6)
    names, pairs = CASES["hydrovsbar"]
    rec, twin = _lone(pkg, n), _lone(pkg, n)
    fs = rec.field_stats(names, pairs, source="hydrovsbar", every=3)
    rec.LBM_timestep(1)
    fs.sample()                                               # by hand after step 1: the count of steps does not move
    rec.LBM_timestep(9)                                       # due after steps 3, 6, 9
    frames = {}
    for s in range(1, 14):
        twin.LBM_timestep(1)
        frames[s] = _frame(pkg, twin, "hydrovsbar", names)
    assert fs.count == 4
    _same(_read(fs), pkg.analysis.field_statistics([frames[s] for s in (1, 3, 6, 9)], pairs), "every = 3")
    first_before = fs.first(0)
    fs.reset()
    assert fs.count == 0
    with pytest.raises(pkg.BflbmError, match="no frame"):
        fs.mean(0)
    rec.LBM_timestep(3)                                       # the count restarted at step 10: due after step 13, which is frame 0
    assert fs.count == 1
    _same(_read(fs), pkg.analysis.field_statistics([frames[13]], pairs), "after reset")
    assert not np.array_equal(fs.first(0), first_before)
    rec.LBM_timestep(3)
    twin.LBM_timestep(3)
    want = pkg.analysis.field_statistics([frames[13], _frame(pkg, twin, "hydrovsbar", names)], pairs)
    _same(_read(fs), want, "second frame after reset")
    rec.close()                                               # detaches: readable, no longer fed
    assert fs._h is not None
    _same(_read(fs), want, "detached")
    with pytest.raises(pkg.BflbmError, match="destroyed"):
        fs.sample()
    fs.close(); twin.close()


def test_refusals_leave_the_owner_untouched(pkg):
    n = (8, 6, 5)
    lbm, twin = _lone(pkg, n), _lone(pkg, n)
    lbm.LBM_timestep(2); twin.LBM_timestep(2)
    bad = [dict(variables=[0], every=-1), dict(variables=[]), dict(variables=list(range(9))),
           dict(variables=[0, 1], pairs=[(0, 1)] * 17),
           dict(variables=[22]), dict(variables=[9], source="hydrovsbar"), dict(variables=[38], source="noise"), dict(variables=[-1]),
           dict(variables=[0, 3, 0]), dict(variables=[0, 1], pairs=[(0, 2)]), dict(variables=[0, 1], pairs=[(-1, 0)]),
           dict(variables=[0], source=3)]
    for kw in bad:
        with pytest.raises((pkg.BflbmError, ValueError)):
            lbm.field_stats(**kw)
    assert not getattr(lbm, "_dependents", [])
    # an open step refuses creation, a frame by hand and reading
    fs = lbm.field_stats(["rho"], [(0, 0)])
    fs.sample()
    lbm.step_boundary()
    for call in (lambda: lbm.field_stats(["rho"]), fs.sample, fs.reset, lambda: fs.mean(0)):
        with pytest.raises(pkg.BflbmError, match="open step"):
            call()
    lbm.step_interior(); lbm.step_finish()
    twin.LBM_timestep(1)
    # reading: what, index and replica out of range, the raw accumulators of an ensemble
    out = np.empty(fs.shape)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    for what, index, replica in [(5, 0, 0), (-1, 0, 0), (1, 1, 0), (4, 1, 0), (1, 0, 1), (1, 0, -2), (0, 0, -1), (2, 0, -1), (3, 0, -1)]:
        assert lbm.lib.bflbm_fstat_get(fs._h, what, index, replica, ptr) != 0, (what, index, replica)
        assert "bflbm_fstat_get" in lbm.lib.bflbm_last_error().decode()
    assert fs.count == 1 and same_doubles(fs.mean(0, replica=-1), 0.0 + fs.sum(0))
    # a replica view and a slab of a decomposed lattice are not owners; a batch has no noise source
    batch = pkg.BatchLBM(n, params=dict(MIXTURE), replicas=2, schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    ring = pkg.RingLBM(8, 8, 8, nslabs=2, devices=(0,), params=pkg.default_params(**MIXTURE), schedule="fused")
    ring.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match="replica of a batch"):
        batch.replicas[0].field_stats(["rho"])
    with pytest.raises(pkg.BflbmError, match="slab of a decomposed lattice"):
        ring.slabs[0].field_stats(["rho"])
    with pytest.raises(pkg.BflbmError, match="noise"):
        batch.field_stats(["fn1"], source="noise")
    assert not getattr(batch, "_dependents", []) and not getattr(ring, "_dependents", [])
    batch.close(); ring.close()
    for a, b in zip(lbm.populations(), twin.populations()):
        assert np.array_equal(a, b)
    assert lbm.steps_done == twin.steps_done == 3
    fs.close(); lbm.close(); twin.close()


# ---- 4. coexistence: three kinds share the scratch state buffer --------------------------------------------------------------
def test_coexists_with_a_spectrum_trace_and_a_mode_trace(pkg):
    n = (8, 8, 8)
    names, pairs = ["rho", "ufx"], [(0, 1), (1, 1)]
    modes = np.array([(1, 0, 0), (0, 1, 1), (1, 1, 1)])
    make = {"spectrum": lambda o: o.spectrum_trace(names, every=1, capacity=6),
            "fstat": lambda o: o.field_stats(names, pairs, every=1),
            "modes": lambda o: o.mode_trace(names, modes, every=1, capacity=6)}

    def read(kind, r):
        return _read(r) if kind == "fstat" else r.read()

    both = _lone(pkg, n)
    together = {k: make[k](both) for k in ("spectrum", "fstat", "modes")}      # creation order: before, the recorder, after
    both.LBM_timestep(6)
    got = {k: read(k, r) for k, r in together.items()}
    both.close()
    for k in make:
        alone = _lone(pkg, n)
        r = make[k](alone)
        alone.LBM_timestep(6)
        want = read(k, r)
        alone.close()
        if k == "fstat":
            _same(got[k], want, "coexistence")
        else:
            assert np.array_equal(got[k][0], want[0]) and same_doubles(got[k][1], want[1]), k


# ---- 5. a batch -------------------------------------------------------------------------------------------------------------
def _batch_params():
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


@pytest.mark.parametrize("source", ["hydrovs", "hydrovsbar"])
def test_batch_replicas_equal_lone_runs_and_the_ensemble(pkg, source):
    n = (8, 6, 5)
    names, pairs = CASES[source]
    names, pairs = names[::-1], [(len(names) - 1 - a, len(names) - 1 - b) for a, b in pairs]     # not in ascending order
    batch = pkg.BatchLBM(n, params=_batch_params(), schedule="fused")
    for v in batch.replicas:
        v.LBM_init_mixture()
    fs = batch.field_stats(names, pairs, source=source, every=2)
    fs.sample()
    batch.LBM_timestep(8)                                     # frames after the steps 0, 2, 4, 6, 8
    assert fs.count == 5 and fs._count()[1] == 3
    reps = []
    for r, p in enumerate(_batch_params()):
        lone = pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule="fused")
        lone.LBM_init_mixture()
        frames = [_frame(pkg, lone, source, names)]
        for _ in range(4):
            lone.LBM_timestep(2)
            frames.append(_frame(pkg, lone, source, names))
        lone.close()
        reps.append(pkg.analysis.field_statistics(frames, pairs))
        _same(_read(fs, r), reps[-1], (source, "replica", r))
    ens = pkg.analysis.field_statistics_ensemble(reps)
    for v in range(len(names)):
        assert same_doubles(fs.mean(v, replica=-1), ens["mean"][v]), v
    for p in range(len(pairs)):
        assert same_doubles(fs.cov(p, replica=-1), ens["cov"][p]), p
    with pytest.raises(pkg.BflbmError, match="ensemble"):
        fs.sum(0, replica=-1)
    batch.close()
    assert same_doubles(fs.cov(0, replica=-1), ens["cov"][0])  # detached, still readable
    fs.close()


# ---- 6. a ring of z-slabs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslabs", [2, 3])
def test_ring_accumulators_equal_the_lone_lattice(pkg, nslabs):
    n = (8, 8, 12)
    cases = {"hydrovs": (["rho", "phi", "rhot"], [(0, 0), (0, 1), (2, 2)]), "noise": (["fn1"], [(0, 0)])}
    ring = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**MIXTURE), schedule="fused")
    ring.LBM_init_mixture()
    lone = _lone(pkg, n)
    recs = {}
    for owner in (ring, lone):
        for source, (names, pairs) in cases.items():
            recs[(owner is ring, source)] = owner.field_stats(names, pairs, source=source, every=1)
            recs[(owner is ring, source)].sample()
        owner.LBM_timestep(4)                                 # 5 frames
    for source in cases:
        got, want = _read(recs[(True, source)]), _read(recs[(False, source)])
        assert want["N"] == 5 and np.abs(want["cov"]).max() > 0
        _same(got, want, (nslabs, source))
    for a, b in zip(ring.populations(), lone.populations()):
        assert np.array_equal(a, b)
    # the lone lattice's own accumulators are the restatement's (test 1); the ring of one slab is the lone recorder
    one = pkg.RingLBM(*n, nslabs=1, devices=(0,), params=pkg.default_params(**MIXTURE), schedule="fused")
    one.LBM_init_mixture()
    fs1 = one.field_stats(*cases["hydrovs"], every=1)
    fs1.sample()
    one.LBM_timestep(4)
    _same(_read(fs1), _read(recs[(False, "hydrovs")]), "ring of one slab")
    ring.close(); lone.close(); one.close()
    _same(_read(recs[(True, "noise")]), _read(recs[(False, "noise")]), "detached ring")
    for r in list(recs.values()) + [fs1]:
        r.close()


# ---- 7. the job flow --------------------------------------------------------------------------------------------------------
def test_job_equilibrium_files_from_the_device_are_byte_identical(pkg, tmp_path):
    common = ["--system", "droplet", "--nx", "16", "--alpha0", "2.0", "--radius", "0.3", "--nsteps", "60", "--plot-int", "10", "--print-int", "0"]
    roots = {flag: str(tmp_path / ("dev" if flag else "disk")) for flag in (True, False)}
    for flag, root in roots.items():
        assert pkg.run_job.main(common + ["--root", root] + (["--eq-device"] if flag else [])) == 0
    sub = "data_droplet_density_1.00_alpha0_2.00_r0.300_size16-16-16"
    for key in ("rho", "phi", "rhot"):
        name = os.path.join(sub, "equilibrium_%s_alpha0_2.00_size16-16-16" % key)
        files = []
        for base, _, fnames in os.walk(os.path.join(roots[False], name)):
            files += [os.path.relpath(os.path.join(base, f), roots[False]) for f in fnames]
        assert len(files) >= 3, files                         # Header, Level_0/Cell_H, Level_0/Cell_D_*
        match, mismatch, errors = filecmp.cmpfiles(roots[False], roots[True], files, shallow=False)
        assert sorted(match) == sorted(files) and not mismatch and not errors, (key, mismatch, errors)
    mean = pkg.plotfile.read_plotfile(os.path.join(roots[True], sub, "equilibrium_rho_alpha0_2.00_size16-16-16"))[0]
    assert mean.shape == (1, 16, 16, 16) and mean.max() > 0.5


# ---- 8. the notebook's statistic on the device --------------------------------------------------------------------------------
def test_noisecovariance_notebook_statistic_on_the_device(pkg):
    """NoiseCovariance.ipynb cell 3 (tests/test_gpu_noise.py::test_noisecovariance_notebook_statistic) without a download
    per frame: 16^3, tau = 1, kBT = 1e-5, alpha0 = 0, 500 steps, then 200 frames every 3 steps of the f momentum-mode
    noise.  The notebook divides the raw sum of squares, so the raw second moment is formed as cov + mean^2 (prod / N is
    the moment about the first frame).  Same 4-sigma bands: the site mean within 0.0065 of 1, the site variance within
    0.0015 of 0.0100; they contain the notebook's 1.00041 and 0.00965."""
    n, frames, kBT, tau = 16, 200, 1e-5, 1.0
    lbm = pkg.BinaryLBM(n, n, n, params=pkg.default_params(kBT=kBT, alpha0=0.0, tau_f=tau, tau_g=tau))
    lbm.LBM_init_mixture()
    lbm.LBM_timestep(500)
    fs = lbm.field_stats(["fn1", "fn2", "fn3"], ["fn1", "fn2", "fn3"], source="noise", every=3)
    lbm.LBM_timestep(3 * frames)
    assert fs.count == frames
    lam_bar = (1.0 / tau) / (1.0 + 0.5 / tau)
    factor1 = 2.0 * lam_bar - lam_bar ** 2
    for a in range(3):
        raw = fs.cov(a) + fs.mean(a) ** 2
        norm = raw / kBT / factor1 / 0.5
        print("mode %d: site mean %.5f, site variance %.5f" % (a + 1, norm.mean(), norm.var()))
        assert abs(norm.mean() - 1.0) < 0.0065, norm.mean()
        assert abs(norm.var() - 0.0100) < 0.0015, norm.var()
    fs.close(); lbm.close()
