"""GPU: the device-side observables on planes of more than 256 blocks, against exact sums.

Every reduction of an observable has two stages: one partial per 256-site block of the padded plane (block_reduce, k_reduce),
then k_plane_partials / k_trace_finish, whose 256 threads each walk a 256-strided subsequence of a
plane's partials (for mass / com_sums the host adds the partials in sequence).  That strided loop runs a second time only
where pitch * ny > 65536; the shapes here are the smallest on either side of it (exact_sums.WIDE_SHAPES):

    512 x 128 x 3     pitch  512, 256 blocks: the last width one pass serves (control)
    4112 x 16 x 3     pitch 4112, 257 blocks: the first second pass, thread 0 alone adds two blocks
    500 x 135 x 4     pitch  512, 270 blocks: a second pass, 12 padded columns per row
    1000 x 141 x 2    pitch 1008, 556 blocks: three passes for threads 0-43, the last block ragged at 48 sites

The state is LBM_init(f0, g0) with f0[i] = w_i rho, g0[i] = w_i phi, rho and phi i.i.d. uniform in [0.5, 1.5): every
site, block and lane carries weight, so a block that is dropped, doubled or read from the wrong place changes a sum by
about 1 / nbx of itself.  The references are the exact sums (exact_sums.exact_moments, integer arithmetic, no rounding)
of the density downloaded once per shape.  No tolerance here is measured.  Each is one of
  * exact_sums.depth_bound of the shape, relative to sum |term|: d u / (1 - d u) for the d roundings a term passes
    through in the order the kernels add (tests/test_exact_sums.py holds the order's numpy restatement against it, and
    shows that a stage 2 cut to its first pass misses it);
  * bit equality (trace against droplet_moments, batch and ring against the lone lattice, interface heights);
  * rtol = 1e-9 of the fits, the tolerance of tests/test_gpu_droplet.py for the same quantities.
Each test prints its largest error / bound."""
import numpy as np
import pytest

import exact_sums as xs
from observable_twins import flow_twin, same_doubles

pytestmark = pytest.mark.gpu

SHAPES = [s for s, _, _ in xs.WIDE_SHAPES]
WIDE = (500, 135, 4)                                # batch and interface traces
RING8, RING13 = (500, 135, 8), (500, 135, 13)       # the ring: 2 slabs of 4 planes; 3 slabs of 4, 4 and 5 planes
BLOB = (1000, 141, 2)                               # the fits
_refs = {}


def _fields(shape, seed=0):
    """rho, phi [nz, ny, nx] to upload: i.i.d. uniform in [0.5, 1.5), a fixed stream per shape and seed."""
    base = 1000 * seed + sum(shape)
    return xs.uniform_field(shape, base), xs.uniform_field(shape, base + 500)


def _populations(ob, rho, phi):
    """f0[i] = w_i rho, g0[i] = w_i phi: at rest, the densities of the resident state are rho and phi up to rounding."""
    w = np.asarray(ob.lattice_tables()[1])[:, None, None, None]
    return np.ascontiguousarray(w * rho), np.ascontiguousarray(w * phi)


def _lone(pkg, ob, shape, schedule=None, seed=0, fields=None):
    lbm = pkg.BinaryLBM(*shape, schedule=schedule)
    lbm.LBM_init(*_populations(ob, *(fields if fields is not None else _fields(shape, seed))))
    return lbm


def _reference(pkg, ob, shape):
    """Once per shape: the densities the device forms from the upload, and their exact sums."""
    if shape not in _refs:
        with _lone(pkg, ob, shape) as lbm:
            rho, phi = lbm.LBM_hydrovars(ncomp=2)
        assert 0.5 <= rho.min() and rho.max() < 1.5 and 0.5 <= phi.min() and phi.max() < 1.5
        assert np.unique(rho).size == rho.size                          # no two sites are equal
        _refs[shape] = dict(rho=rho, phi=phi, plain=xs.exact_moments(rho), weighted=xs.exact_moments(rho, weighted=True),
                            above=xs.exact_moments(rho, threshold=1.0), phi_mass=xs.exact_moments(phi)[0][0])
    return _refs[shape]


def _within(got, exact, abs_sum, bound, what):
    """Every got[k] within bound * sum |term| of exact[k]; returns the largest error / bound."""
    ratios = [xs.ratio_to_bound(g, e, a, bound) for g, e, a in zip(got, exact, abs_sum)]
    print(f"{what}: bound {bound:.3e}, error / bound {max(ratios):.4f} (worst entry {int(np.argmax(ratios))})")
    assert max(ratios) <= 1.0, (what, ratios)
    return max(ratios)


def _com_within(got, moments, n, bound, what):
    """got[d] within `bound`, relative, of the exact centre of mass (unit-box cell-centre coordinates)."""
    ratios = [xs.ratio_to_bound(g, e, e, bound) for g, e in zip(got, xs.exact_com(moments, n))]
    print(f"{what}: bound {bound:.3e}, error / bound {max(ratios):.4f}")
    assert max(ratios) <= 1.0, (what, ratios)


# ---- 1. droplet moments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_droplet_moments_against_exact_sums(pkg, ob, shape):
    ref = _reference(pkg, ob, shape)
    bound = xs.depth_bound("two_stage", *shape)
    with _lone(pkg, ob, shape) as lbm:
        m = lbm.droplet_moments()
    _within(m[:10], *ref["plain"], bound, f"{shape} moments")
    _within(m[10:], *ref["weighted"], bound, f"{shape} weighted moments")
    an = pkg.analysis
    _com_within(an.com_from_moments(m, shape), ref["plain"][0], shape, 2 * bound, f"{shape} com_from_moments")
    _com_within(an.com_from_moments(m, shape, weighted=True), ref["weighted"][0], shape, 2 * bound, f"{shape} weighted com_from_moments")


# ---- 2. mass and centre of mass: the host adds the block sums -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_mass_and_com_against_exact_sums(pkg, ob, shape):
    ref = _reference(pkg, ob, shape)
    exact, abs_sum = ref["plain"]
    bound = xs.depth_bound("host_blocks", *shape)
    with _lone(pkg, ob, shape) as lbm:
        mass, sums, com = lbm.mass(), lbm.com_sums(), lbm.update_com()
    _within(mass, [exact[0], ref["phi_mass"]], [abs_sum[0], ref["phi_mass"]], bound, f"{shape} mass (rho, phi)")
    _within(sums, exact[:4], abs_sum[:4], bound, f"{shape} com_sums")
    # update_com: the quotient of two of these sums, in cell indices.  A priori it is good to 2 bound + u; the single bound
    # is what is asserted, the stricter claim (d counts every one of the nbx * nz additions of the host loop)
    want = [exact[1 + d] / exact[0] for d in range(3)]
    ratios = [xs.ratio_to_bound(g, e, e, bound) for g, e in zip(com, want)]
    print(f"{shape} update_com: bound {bound:.3e}, error / bound {max(ratios):.4f}")
    assert max(ratios) <= 1.0, ratios


# ---- 3. the lone trace ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("shape", SHAPES)
def test_lone_trace_equals_droplet_moments(pkg, ob, shape, schedule):
    """threshold = -inf: two samples one step apart (the slot advances) equal droplet_moments of the same states bit for
    bit, and the second, whose density no test field prescribes, lies within the bound of its own exact sums."""
    nsites = shape[0] * shape[1] * shape[2]
    with _lone(pkg, ob, shape, schedule) as lbm:
        assert lbm.resolved_schedule() == schedule
        tr = lbm.trace(every=1, capacity=2, threshold=-np.inf)
        tr.sample()
        want = [lbm.droplet_moments()[:10]]
        lbm.LBM_timestep(1)
        want.append(lbm.droplet_moments()[:10])
        steps, rec = tr.read()
        rho1 = lbm.LBM_hydrovars(ncomp=1)[0]
    assert steps[:, 0].tolist() == [0, 1] and rec.shape == (2, 1, 12)
    assert np.all(np.isfinite(rec)) and not np.array_equal(want[0], want[1])
    for k in range(2):
        assert np.array_equal(rec[k, 0, :10], want[k]), (k, rec[k, 0, :10] - want[k])
    assert np.all(rec[:, 0, 11] == nsites) and np.array_equal(rec[:, 0, 10], rec[:, 0, 0])
    bound = xs.depth_bound("two_stage", *shape)
    _within(rec[0, 0, :10], *_reference(pkg, ob, shape)["plain"], bound, f"{shape} {schedule} trace, step 0")
    _within(rec[1, 0], *xs.exact_moments(rho1, threshold=-np.inf), bound, f"{shape} {schedule} trace, step 1")


@pytest.mark.parametrize("shape", SHAPES)
def test_threshold_trace_against_exact_sums(pkg, ob, shape):
    ref = _reference(pkg, ob, shape)
    exact, abs_sum = ref["above"]
    with _lone(pkg, ob, shape) as lbm:
        tr = lbm.trace(every=1, capacity=1, threshold=1.0)
        tr.sample()
        rec = tr.read()[1][0, 0]
    nsites = ref["rho"].size
    assert 0.45 * nsites < exact[11] < 0.55 * nsites                    # about half the cells pass
    assert rec[11] == exact[11] == int((ref["rho"] > 1.0).sum())
    _within(rec[:11], exact[:11], abs_sum[:11], xs.depth_bound("two_stage", *shape), f"{shape} trace above 1.0")
    assert exact[10] == ref["plain"][0][0]                              # record 10 is the mass of every cell


# ---- 4. the batch trace ---------------------------------------------------------------------------------------------------
def test_batch_trace_equals_lone_lattices(pkg, ob):
    """Two replicas with different fields: replica r's blocks lie behind replica 0's in the stage buffer."""
    fields = [_fields(WIDE, seed=s) for s in (1, 2)]
    batch = pkg.BatchLBM(WIDE, params={}, replicas=2, schedule="two_pass")
    for rep, fl in zip(batch.replicas, fields):
        rep.LBM_init(*_populations(ob, *fl))
    tr = batch.trace(every=1, capacity=2, threshold=-np.inf)
    tr.sample()
    batch.LBM_timestep(1)
    steps, rec = tr.read()
    batch.close()
    assert rec.shape == (2, 2, 12) and steps.tolist() == [[0, 0], [1, 1]]
    bound = xs.depth_bound("two_stage", *WIDE)
    for r, fl in enumerate(fields):
        with _lone(pkg, ob, WIDE, "two_pass", fields=fl) as lone:
            lt = lone.trace(every=1, capacity=2, threshold=-np.inf)
            lt.sample()
            rho0 = lone.LBM_hydrovars(ncomp=1)[0]
            lone.LBM_timestep(1)
            lrec = lt.read()[1]
        assert np.array_equal(rec[:, r], lrec[:, 0]), (r, rec[:, r] - lrec[:, 0])
        _within(rec[0, r], *xs.exact_moments(rho0, threshold=-np.inf), bound, f"{WIDE} batch trace, replica {r}")
    assert not np.array_equal(rec[:, 0], rec[:, 1])


# ---- 5. the ring ------------------------------------------------------------------------------------------------------------
def test_a_ring_needs_four_planes_per_slab(pkg):
    """Why the three-slab case below has 13 planes: 500 x 135 x 8 cannot be cut into three slabs."""
    with pytest.raises(pkg.BflbmError, match="at least 4 planes"):
        pkg.RingLBM(*RING8, nslabs=3, devices=(0,))


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("shape,nslabs", [(RING8, 2), (RING13, 3)])
def test_ring_observables_equal_the_lone_lattice(pkg, ob, shape, nslabs, schedule):
    """The ring's stage buffer takes slab k's blocks at plane z0 of the slab (peer copies of nzl * nbx * 12 doubles); with
    the exact schedules its trace equals the lone trace bit for bit, and so do its droplet moments, whose planes
    slab_reduce adds in the lone order whatever the decomposition."""
    f0, g0 = _populations(ob, *_fields(shape))
    ring = pkg.RingLBM(*shape, nslabs=nslabs, devices=(0,), schedule=schedule)
    assert [s.nzl for s in ring.slabs] == {2: [4, 4], 3: [4, 4, 5]}[nslabs]
    ring.LBM_init(f0, g0)
    lone = pkg.BinaryLBM(*shape, schedule=schedule)
    lone.LBM_init(f0, g0)
    out = []
    for o in (ring, lone):
        tr = o.trace(every=1, capacity=2, threshold=-np.inf)
        tr.sample()
        first = (o.droplet_moments(), o.mass(), o.update_com())
        o.LBM_timestep(1)
        out.append((tr.read(), first, o.droplet_moments()))
    ring.close(); lone.close()
    ((rs, rrec), (rm, rmass, rcom), rm1), ((ls, lrec), (lm, lmass, lcom), lm1) = out
    assert rs[:, 0].tolist() == ls[:, 0].tolist() == [0, 1] and np.all(np.isfinite(rrec))
    assert np.array_equal(rrec, lrec), rrec - lrec
    assert np.array_equal(rm, lm) and np.array_equal(rm1, lm1)
    assert np.array_equal(rrec[0, 0, :10], rm[:10]) and np.array_equal(rrec[1, 0, :10], rm1[:10])
    ref = _reference(pkg, ob, shape)
    bound = xs.depth_bound("two_stage", *shape, nslabs=nslabs)
    _within(rm[:10], *ref["plain"], bound, f"{shape} / {nslabs} ring moments")
    _within(rm[10:], *ref["weighted"], bound, f"{shape} / {nslabs} ring weighted moments")
    exact, abs_sum = ref["plain"]
    hb = xs.depth_bound("host_blocks", *shape, nslabs=nslabs)
    _within(rmass, [exact[0], ref["phi_mass"]], [abs_sum[0], ref["phi_mass"]], hb, f"{shape} / {nslabs} ring mass (rho, phi)")
    want = [exact[1 + d] / exact[0] for d in range(3)]
    assert max(xs.ratio_to_bound(g, e, e, hb) for g, e in zip(rcom, want)) <= 1.0


# ---- 6. the interface trace -----------------------------------------------------------------------------------------------
def test_interface_trace_on_a_wide_plane(pkg, ob):
    """rho rises through the level between planes 1 and 2 and phi falls through it there, by another amount in every
    column: the dense [2][ny][nx] heights equal the restatement, so no padded column was taken for a site."""
    nx, ny, nz = WIDE
    u, v = _fields(WIDE, seed=3)                                        # in [0.5, 1.5)
    low, high = 0.1 + 0.5 * u, 0.9 + 0.5 * v                            # [0.35, 0.85) and [1.15, 1.65)
    rho = np.where(np.arange(nz)[:, None, None] < 2, low, high)
    phi = np.where(np.arange(nz)[:, None, None] < 2, high, low)
    level = 1.0
    with _lone(pkg, ob, WIDE, fields=(rho, phi)) as lbm:
        traces = [lbm.interface_trace(level, field=f, every=1, capacity=1) for f in ("rho", "phi")]
        for tr in traces:
            tr.sample()
        dens = lbm.LBM_hydrovars_density(ncomp=2)
        got = [tr.read()[1] for tr in traces]
        assert all(tr.geometry()[:2] == (nx, ny) for tr in traces)
    for k, (h, d) in enumerate(zip(got, dens)):
        assert h.shape == (1, 1, 2, ny, nx)
        want = pkg.analysis.interface_heights(d, level)
        crossing, other = want[k], want[1 - k]                          # rho rises (0), phi falls (1)
        assert np.all((1.0 < crossing) & (crossing < 2.0)) and np.all(np.isnan(other))
        assert np.unique(crossing).size > 0.99 * nx * ny                # another height in every column
        assert same_doubles(h[0, 0], want), ("rho", "phi")[k]


# ---- 7. the fits ------------------------------------------------------------------------------------------------------------
def _blob():
    """rho = 0.1 + 1/2 (1 + tanh((R - r) / sqrt(2 W))) about the box centre in unit-box coordinates, r measured with the y
    axis stretched: an ellipsoid, which the spherical profile of the fits cannot match, so the cost stays far from zero.
    The maximum lies on row ny / 2 = 70, block 70 * 1008 / 256 = 275: beyond the first pass of stage 2."""
    nx, ny, nz = BLOB
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + ((y - 0.5) / 1.3) ** 2 + (z - 0.5) ** 2)
    rho = 0.1 + 0.5 * (1.0 + np.tanh((0.25 - r) / np.sqrt(2 * 0.002)))
    return rho, 1.2 - rho


def test_fits_on_a_wide_plane(pkg, ob):
    an = pkg.analysis
    with _lone(pkg, ob, BLOB, fields=_blob()) as lbm:
        rho = lbm.LBM_hydrovars(ncomp=1)[0]
        p = np.array(lbm.fit_droplet())
        cost_dev = lbm.last_fit["cost"]
        W, R, und = lbm.fit_droplet_flow(nstep=4, step_window=2, undul_ratio=1.0)
        retries = lbm.last_fit["retries"]
    nbx = xs.blocks_per_plane(*BLOB[:2])
    peak = np.unravel_index(np.argmax(rho), rho.shape)
    assert (peak[1] * xs.pitch_of(BLOB[0]) + peak[2]) // 256 >= 256 and nbx == 556     # the maximum: beyond the first pass
    vals, r = an.radial_profile(np.ascontiguousarray(rho.transpose(2, 1, 0)))
    cost = ((vals - (p[0] - (p[0] - p[1]) / 2 * (1 + np.tanh((r - p[2]) / p[3])))) ** 2).sum()
    print(f"{BLOB} fit_droplet: parameters {p}, cost {cost_dev!r} against numpy {cost!r}")
    assert cost > 1e-6 * rho.size                                       # far from zero: the comparison is about something
    np.testing.assert_allclose(cost_dev, cost, rtol=1e-9)
    (Wt, Rt), undt = flow_twin(pkg, rho, 0.02, 0.3, 4, 2)               # the defaults of bflbm_flowfit_opts
    print(f"{BLOB} fit_droplet_flow: (W, R) = {(W, R)!r} against the twin {(Wt, Rt)!r}")
    assert retries == 0 and np.all(undt <= 1.0) and und <= 1.0
    np.testing.assert_allclose([W, R], [Wt, Rt], rtol=1e-9)


# ---- 8. the total-density bound of `auto`: the NaN-propagating maximum, the host over all blocks ----------------------------
ABSMAX_SHAPES = [(4112, 16, 3), (1000, 141, 2)]     # 257 blocks per plane; 556 blocks, the last one ragged at 48 sites


def _peaked(ob, shape, nan=False):
    """The module's uniform upload with rho of the last site (nx-1, ny-1, nz-1) scaled by 5, so that rho + phi >= 3 there
    and < 3 everywhere else: the maximum lives in the last block of the last plane.  nan: that site's f0[0] is NaN."""
    rho, phi = _fields(shape)
    rho = rho.copy()
    rho[-1, -1, -1] *= 5.0
    f0, g0 = _populations(ob, rho, phi)
    if nan:
        f0[0, -1, -1, -1] = np.nan
    return f0, g0


def _assert_peak(total_max, rho, phi):
    total = np.abs(rho + phi)
    peak = np.unravel_index(np.argmax(total), total.shape)
    print(f"{rho.shape[::-1]} state_total_max {total_max!r} against the downloaded densities {total.max()!r} at (z, y, x) = {peak}")
    assert peak == tuple(n - 1 for n in total.shape) and total.max() >= 3.0 > np.partition(total.ravel(), -2)[-2]
    assert total_max == total.max(), (total_max, total.max())           # bit for bit: a maximum rounds nothing


@pytest.mark.parametrize("shape", ABSMAX_SHAPES)
def test_state_total_max_on_a_wide_plane(pkg, ob, shape):
    assert xs.blocks_per_plane(*shape[:2]) > 256
    with pkg.BinaryLBM(*shape) as lbm:
        lbm.LBM_init(*_peaked(ob, shape))
        m = lbm.state_total_max
        rho, phi = lbm.LBM_hydrovars(ncomp=2)
    _assert_peak(m, rho, phi)


def test_state_total_max_of_a_ring_is_the_global_one(pkg, ob):
    """The large site lies in slab 1; every slab resolves `auto` on the whole lattice's maximum."""
    ring = pkg.RingLBM(*RING8, nslabs=2, devices=(0,))
    ring.LBM_init(*_peaked(ob, RING8))
    ms = [s.state_total_max for s in ring.slabs]
    rho, phi = ring.LBM_hydrovars(ncomp=2)
    ring.close()
    assert ms[0] == ms[1]
    _assert_peak(ms[0], rho, phi)


@pytest.mark.parametrize("shape", ABSMAX_SHAPES)
def test_a_nan_in_the_last_block_keeps_auto_on_an_exact_schedule(pkg, ob, shape):
    with pkg.BinaryLBM(*shape) as lbm:
        lbm.LBM_init(*_peaked(ob, shape, nan=True))
        assert lbm.state_total_max == np.inf
        assert lbm.resolved_schedule() in ("two_pass", "fused")
