"""GPU: ensemble structure factors (csrc/bflbm_batch_sf.h).  One accumulator observes, transforms and accumulates every
replica of a batch with one launch each; the stacked getters of BatchLBM use the same observation kernel.
The observation is compared bit for bit with the views' own getters (k_observe), the spectra with the host definition
(structfact.StructFact, numpy FFT) to the tolerance of tests/test_gpu_structfact.py: two FFT libraries agree to rounding,
1e-11 of the largest |S| of each pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 16), (12, 10, 14), (9, 7, 5)]       # odd nx (half spectrum nx/2+1), a padded pitch, nz < 8


def _agree(dev, host):
    scale = np.abs(host).max(axis=(1, 2, 3), keepdims=True)
    scale[scale == 0] = 1.0
    assert np.abs(dev - host).max() <= 1e-11 * scale.max() or np.all(np.abs(dev - host) <= 1e-11 * scale)


def _params(quiet=False):
    return [dict(alpha0=a, tau_f=t, tau_g=t, kBT=0.0 if quiet else k, seed=s)
            for a, t, k, s in zip((0.0, 1.0, 1.5), (1.0, 0.8, 0.5), (1e-5, 2e-5, 1e-5), (101, 202, 303))]


def _batch(pkg, n, schedule=None, quiet=False):
    """B = 3 replicas that differ in parameters, seed and step counter (noise index, record and buffer parity)."""
    batch = pkg.BatchLBM(n, params=_params(quiet), schedule=schedule)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.replicas[1].set_steps_done(1000)
    return batch


# ---- 1. the observation kernel, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("quiet", [False, True], ids=["noise", "quiet"])
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("n", SHAPES)
def test_stacked_getters_equal_the_views_bit_for_bit(pkg, n, schedule, quiet):
    batch = _batch(pkg, n, schedule, quiet)
    views = batch.replicas

    def compare(first):
        # first: who observes first decides whether the batch call finds the densities valid, stale or mixed
        if first == "views":
            want = np.stack([v.LBM_hydrovars() for v in views])
            got = batch.LBM_hydrovars()
        else:
            if first == "view 0":
                views[0].LBM_hydrovars()
            got = batch.LBM_hydrovars()
            want = np.stack([v.LBM_hydrovars() for v in views])
        assert got.shape == (3, 22, n[2], n[1], n[0])
        assert np.array_equal(got, want)
        assert np.array_equal(batch.LBM_hydrovars_density(), np.stack([v.LBM_hydrovars_density() for v in views]))
        for ncomp in (22, 9, 5):
            assert np.array_equal(batch.LBM_hydrovars(ncomp), np.stack([v.LBM_hydrovars(ncomp=ncomp) for v in views]))
        assert np.array_equal(batch.LBM_hydrovars_density(5), np.stack([v.LBM_hydrovars_density()[:5] for v in views]))

    compare("batch")                                   # k = 0 right after the inits: the device records are stale
    for nsteps, first in ((1, "batch"), (1, "views"), (5, "view 0")):     # after 1, 2 and 7 steps: both parities of k
        batch.LBM_timestep(nsteps)
        compare(first)
    assert [v.steps_done for v in views] == [7, 1007, 7]
    batch.close()


# ---- 2. spectra against the host definition ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_batch_structure_factor_matches_host(pkg, n):
    batch = _batch(pkg, n)
    names = pkg.plotfile.variable_names(22)
    hosts = [pkg.structfact.StructFact(names) for _ in batch.replicas]
    dev = pkg.structfact.BatchStructFact(batch, names, every=0)
    assert dev.pair_names() == hosts[0].pair_names() and len(dev.pairs) == 22
    batch.LBM_timestep(20)
    for _ in range(3):
        batch.LBM_timestep(5)
        for h, v in zip(hosts, batch.replicas):
            h.fort_structure(v.LBM_hydrovars(), 0)
        dev.fort_structure()
    assert dev.nsamples == 3
    auto = [i for i, (a, b) in enumerate(dev.pairs) if a == b]
    for zero_avg in (1, 0):
        hm = [h.mean(zero_avg) for h in hosts]
        stacked = dev.means(zero_avg)
        assert stacked.shape == (3, 22, n[2], n[1], n[0])
        for r in range(3):
            d = dev.mean(zero_avg, replica=r)
            assert np.array_equal(d, stacked[r])
            _agree(d.real, hm[r].real)
            _agree(d.imag, hm[r].imag)
            _agree(dev.magnitude(zero_avg, replica=r), np.abs(hm[r]))
        ens = np.mean(hm, axis=0)
        d = dev.mean(zero_avg)
        _agree(d.real, ens.real)
        _agree(d.imag, ens.imag)
        _agree(dev.magnitude(zero_avg), np.abs(ens))
    # auto-correlations are real and non-negative, per replica and in the ensemble
    for d in [dev.mean(0)] + [dev.mean(0, replica=r) for r in range(3)]:
        assert np.all(d[auto].real >= 0) and np.abs(d[auto].imag).max() <= 1e-25
    # reset restarts the average
    dev.fort_structure(reset=1)
    assert dev.nsamples == 1
    for r, (h, v) in enumerate(zip(hosts, batch.replicas)):
        h.fort_structure(v.LBM_hydrovars(), 1)
        _agree(dev.mean(1, replica=r).real, h.mean(1).real)
        _agree(dev.mean(1, replica=r).imag, h.mean(1).imag)
    dev.reset()
    assert dev.nsamples == 0
    dev.close(); batch.close()


# ---- 3. hydrovsbar -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_batch_structure_factor_of_hydrovsbar(pkg, n):
    batch = _batch(pkg, n)
    views = batch.replicas
    names = pkg.plotfile.variable_names(9)
    dev = batch.structfact(names, lb_hydrovars=True)                # pairs within the 9 names only
    hosts = [pkg.structfact.StructFact(names) for _ in views]
    assert 0 < len(dev.pairs) < 22 and dev.pair_names() == hosts[0].pair_names()
    batch.LBM_timestep(11)
    dev.fort_structure()                                            # the views' densities are stale here and stay so
    for h, v in zip(hosts, views):
        h.fort_structure(v.LBM_hydrovars_density(), 0)
    batch.LBM_timestep(3)
    for h, v in zip(hosts, views):
        h.fort_structure(v.LBM_hydrovars_density(), 0)
    before = [v.LBM_hydrovars() for v in views]
    dev.fort_structure()
    after = [v.LBM_hydrovars() for v in views]
    assert dev.nsamples == 2
    for x, y in zip(before, after):                                 # a frame leaves what the views observe unchanged
        assert np.array_equal(x, y)
    for r, h in enumerate(hosts):
        for zero_avg in (1, 0):
            _agree(dev.mean(zero_avg, replica=r).real, h.mean(zero_avg).real)
            _agree(dev.mean(zero_avg, replica=r).imag, h.mean(zero_avg).imag)
    _agree(dev.mean(1).real, np.mean([h.mean(1) for h in hosts], axis=0).real)
    dev.close(); batch.close()


# ---- 4. attached sampling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SHAPES)
def test_attached_frames_equal_manual_frames(pkg, n):
    names = pkg.plotfile.variable_names(22)
    a, b = _batch(pkg, n), _batch(pkg, n)
    sa = a.structfact(names, every=5)
    sb = b.structfact(names, every=0)
    a.LBM_timestep(20)
    for _ in range(4):
        b.LBM_timestep(5)
        sb.fort_structure()
    assert sa.nsamples == 4 and sb.nsamples == 4
    ma, mb = sa.means(0), sb.means(0)
    for r in range(3):
        _agree(ma[r].real, mb[r].real)
        _agree(ma[r].imag, mb[r].imag)
    # a manual frame on an attached accumulator does not move the count; reset restarts it
    sa.fort_structure()
    assert sa.nsamples == 5
    sa.reset()
    a.LBM_timestep(3)
    assert sa.nsamples == 0
    a.LBM_timestep(2)
    assert sa.nsamples == 1
    b.LBM_timestep(5)
    sb.fort_structure(reset=1)
    for r in range(3):
        _agree(sa.mean(0, replica=r).real, sb.mean(0, replica=r).real)
    for x in (sa, sb, a, b):
        x.close()


# ---- 5. the accumulator changes nothing the batch computes ---------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_attached_accumulator_changes_nothing(pkg, schedule):
    n = (12, 10, 14)
    a, b = _batch(pkg, n, schedule), _batch(pkg, n, schedule)
    sf = a.structfact(pkg.plotfile.variable_names(22), every=1)
    ta, tb = a.trace(every=2, capacity=8), b.trace(every=2, capacity=8)
    a.LBM_timestep(12); b.LBM_timestep(12)
    assert sf.nsamples == 12
    (fa, ga), (fb, gb) = a.populations(), b.populations()
    assert np.array_equal(fa, fb) and np.array_equal(ga, gb)
    assert [v.steps_done for v in a.replicas] == [v.steps_done for v in b.replicas] == [12, 1012, 12]
    (sa, ra), (sb, rb) = ta.read(), tb.read()
    assert ra.shape[0] == 6 and np.array_equal(sa, sb) and np.array_equal(ra, rb)
    a.LBM_timestep(1); b.LBM_timestep(1)
    assert np.array_equal(a.populations()[0], b.populations()[0])
    for x in (sf, ta, tb, a, b):
        x.close()


# ---- 6. lifetime and refusals on the device ------------------------------------------------------------------------------------
def test_lifetime_and_refusals(pkg):
    n = (9, 7, 5)
    batch = _batch(pkg, n)
    sf = batch.structfact(pkg.plotfile.variable_names(22), every=1)
    sb = batch.structfact(pkg.plotfile.variable_names(9), lb_hydrovars=True, every=1)
    batch.LBM_timestep(4)
    assert sf.nsamples == 4 and sb.nsamples == 4                      # two accumulators on one batch both advance
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_sf_get"):
        sf.mean(replica=3)
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_sf_get"):
        sf._get(3, 1)
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_get_hydrovs"):
        batch.LBM_hydrovars(23)
    with pytest.raises(pkg.BflbmError, match="hydrovsbar"):
        pkg.structfact.BatchStructFact(batch, pkg.plotfile.variable_names(22), lb_hydrovars=True)
    before, ens, mag = sf.means(1), sf.mean(1), sf.magnitude(1)
    sb.close()
    batch.close()                                                      # the batch first: the accumulator is detached
    assert sf._h is not None and sf.nsamples == 4
    assert np.array_equal(sf.means(1), before) and np.array_equal(sf.mean(1), ens) and np.array_equal(sf.magnitude(1), mag)
    with pytest.raises(pkg.BflbmError, match="bflbm_batch_sf_accumulate"):
        sf.fort_structure()
    sf.close()
    sf.close()


def test_plotfile_of_the_ensemble_mean(pkg, tmp_path):
    batch = _batch(pkg, (12, 10, 14))
    sf = batch.structfact(pkg.plotfile.variable_names(22), every=2)
    batch.LBM_timestep(6)
    s = sf.write_plotfile(6, 6.0, str(tmp_path / "plt_SF"), zero_avg=1)
    assert np.array_equal(s, sf.mean(1))
    mag, hdr = pkg.plotfile.read_plotfile(str(tmp_path / "plt_SF_mag000000006"))
    assert hdr["names"] == sf.pair_names() and np.array_equal(mag, sf.magnitude(1))
    batch.close()
    sf.close()


# ---- 7. the ensemble statistic the notebooks read ------------------------------------------------------------------------------
def test_ensemble_structure_factor_is_flat(pkg):
    """Mixture.ipynb cell 2 on an ensemble: 4 replicas of 32^3 (kBT = 1e-5, alpha0 = 0, tau = 1, seeds 4242 + r), 2000
    steps, then a frame every 25 steps over 375 steps: the 60 frames of tests/test_gpu_noise.py::
    test_structure_factor_is_flat (15 x 4, independent replicas instead of 25 steps apart), the same estimator
    (hydrovsbar, k = 0 removed) and that test's overall bands: S_rho cs2 / kBT within 0.02, S_u / kBT within 0.03 of 1."""
    n, kBT, cs2 = 32, 1e-5, 1.0 / 3.0
    batch = pkg.BatchLBM(n, params=dict(kBT=kBT, alpha0=0.0, tau_f=1.0, tau_g=1.0, seed=4242), replicas=4)
    for v in batch.replicas:
        v.LBM_init_mixture()
    batch.LBM_timestep(2000)
    sf = batch.structfact(pkg.plotfile.variable_names(9), lb_hydrovars=True, every=25)
    batch.LBM_timestep(375)
    assert sf.nsamples == 15
    pairs = {p: i for i, p in enumerate(sf.pairs)}
    s = sf.mean(zero_avg=1).real
    k1 = np.fft.fftshift(np.fft.fftfreq(n) * n)
    mask = (k1[:, None, None] ** 2 + k1[None, :, None] ** 2 + k1[None, None, :] ** 2) > 0
    s_rho = s[pairs[(0, 0)]][mask].mean() * cs2 / kBT
    s_u = np.mean([s[pairs[(c, c)]][mask].mean() for c in (2, 3, 4)]) / kBT
    print("ensemble S_rho cs2/kBT = %.5f, S_u/kBT = %.5f" % (s_rho, s_u))
    assert abs(s_rho - 1.0) < 0.02, s_rho
    assert abs(s_u - 1.0) < 0.03, s_u
    sf.close(); batch.close()
