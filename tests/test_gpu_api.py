"""GPU: behaviour of the C-ABI beyond the arithmetic -- error conventions, parameter edits between
steps (the reference edits source-level globals between runs), step protocol guards."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_parameter_edit_between_steps(pkg, ob):
    """ReadMe.ipynb workflow: relax at kBT=0, then switch noise on and keep going (same populations)."""
    n = (8, 8, 8)
    lbm = pkg.BinaryLBM(*n, params=pkg.default_params(alpha0=2.0))
    ref = ob.OracleLattice(*n, params=ob.default_params(alpha0=2.0))
    lbm.LBM_init_droplet(0.3)
    ref.init_droplet(0.3)
    lbm.LBM_timestep(3)
    for _ in range(3):
        ref.timestep()
    lbm.set_params(kBT=2e-5, alpha0=1.5, tau_f=0.7)
    ref.p.kBT, ref.p.alpha0, ref.p.tau_f = 2e-5, 1.5, 0.7
    ref.refresh()                      # noise/hydrovs of the current state under the new parameters
    assert np.array_equal(lbm.LBM_hydrovars(), ref.h)
    lbm.LBM_timestep(3)
    for _ in range(3):
        ref.timestep()
    f, g = lbm.populations()
    assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g)
    assert lbm.steps_done == 6
    lbm.close()


def test_error_conventions(pkg):
    lib = pkg._lib.load()
    lbm = pkg.BinaryLBM(8, 8, 8)
    lbm.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError):
        lbm.LBM_timestep(-1)
    lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="already open"):
        lbm.step_boundary()
    with pytest.raises(pkg.BflbmError, match="open step"):
        lbm.populations()
    with pytest.raises(pkg.BflbmError, match="open step"):
        lbm.LBM_hydrovars()
    lbm.step_interior()
    lbm.step_finish()
    with pytest.raises(pkg.BflbmError, match="no open step"):
        lbm.step_finish()
    with pytest.raises(pkg.BflbmError, match="single slab"):
        lbm.halo_pack(0, 0, 1)
    # bad FAB: valid region outside the allocated box
    fab = pkg.make_fab((0, 0, 0), (7, 7, 7), (0, 0, 0), (8, 7, 7))
    out = np.zeros((9, 8, 8, 8))
    with pytest.raises(pkg.BflbmError, match="valid region"):
        lbm.LBM_hydrovars_density(out, fab)
    with pytest.raises(pkg.BflbmError):
        lbm.set_schedule(7)
    lbm.set_schedule("auto")
    with pytest.raises(TypeError):
        lbm.upload(np.zeros((19, 8, 8, 8), dtype=np.float32), np.zeros((19, 8, 8, 8)))
    assert lbm.steps_done == 1
    lbm.close()
    # multi-slab context: several steps per call are refused (a halo exchange is needed in between)
    slab = pkg.BinaryLBM(8, 8, 8, z0=0, z1=4, rank=0, nranks=2)
    slab.LBM_init_mixture()
    with pytest.raises(pkg.BflbmError, match="halo exchange"):
        slab.LBM_timestep(2)
    assert slab.halo_bytes() == 38 * 8 * 8 * 8
    slab.close()


def test_an_open_step_pins_what_it_runs(pkg, ob):
    """bflbm_step_boundary resolves the schedule and the step runs it with the parameters it started with: the calls that
    could change either are refused until bflbm_step_finish, and the step then completes as if they had not been made."""
    n = (16, 16, 16)
    lbm = pkg.BinaryLBM(*n, schedule="fused")
    ref = ob.OracleLattice(*n)
    lbm.LBM_init_stripe(0.5)
    ref.init_stripe(0.5)
    lbm.step_boundary()
    noise = np.zeros((19,) + n)
    eq = np.ones(n)
    for call in (lambda: lbm.set_params(alpha0=1.0, kBT=1e-5), lambda: lbm.set_schedule("two_pass"),
                 lambda: lbm.inject_noise(noise, noise), lambda: lbm.inject_noise(None, None),
                 lambda: lbm.set_state_total_max(100.0), lambda: lbm.set_ref_state(eq, eq, 2 * eq, (8., 8., 8.)),
                 lambda: lbm.disable_ref_state()):
        with pytest.raises(pkg.BflbmError, match="inside an open step"):
            call()
    lbm.step_interior()
    lbm.step_finish()
    ref.timestep()
    f, g = lbm.populations()
    assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g)
    assert lbm.resolved_schedule() == "fused" and lbm.state_total_max < 0 and not lbm.ref_state_active
    lbm.close()


@pytest.mark.parametrize("between", ["fused_step", "set_steps_done"])
def test_handover_frames_are_not_reused_across_an_exact_step_or_a_moved_counter(pkg, between):
    """Frames describe the state of the hand-over step that wrote them.  After an exact step, or after the step counter was
    set, the next hand-over step has none and pulls every ring: it equals one fused step from the same state, bit for bit."""
    n = (128, 16, 32)
    lbm = pkg.BinaryLBM(*n, schedule="handover")
    assert lbm.resolved_schedule() == "handover"
    lbm.LBM_init_droplet(0.2)
    lbm.LBM_timestep(3)
    if between == "fused_step":
        lbm.set_schedule("fused")
        lbm.LBM_timestep(1)
        lbm.set_schedule("handover")
    else:
        lbm.set_steps_done(lbm.steps_done)
    f0, g0 = lbm.populations()
    steps = lbm.steps_done
    lbm.LBM_timestep(1)
    other = pkg.BinaryLBM(*n, schedule="fused")
    other.LBM_init(f0, g0)
    other.set_steps_done(steps)
    other.LBM_timestep(1)
    f, g = lbm.populations()
    fo, go = other.populations()
    assert np.array_equal(f, fo) and np.array_equal(g, go)
    lbm.close()
    other.close()


def test_partial_box_download_only_touches_its_cells(pkg, ob):
    """A FAB covering only part of the lattice (and sticking out of it) gets only its overlap."""
    n = (8, 8, 8)
    lbm = pkg.BinaryLBM(*n)
    ref = ob.OracleLattice(*n)
    lbm.LBM_init_droplet(0.3)
    ref.init_droplet(0.3)
    lo, hi = (4, -2, 2), (9, 5, 6)                 # sticks out in x (hi) and y (lo)
    shp = (9, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    out = np.full(shp, -1.0)
    lbm.LBM_hydrovars_density(out, pkg.make_fab(lo, hi))
    exp = np.full(shp, -1.0)
    exp[:, :, 2:, :4] = ref.hbar[:9, 2:7, 0:6, 4:8]
    assert np.array_equal(out, exp)
    lbm.close()


def test_device_bytes_and_timer(pkg):
    lbm = pkg.BinaryLBM(32, 32, 32)
    assert lbm.device_bytes() >= 2 * 38 * 32 ** 3 * 8
    lbm.LBM_init_stripe(0.5)
    lbm.timer_start()
    lbm.LBM_timestep(10)
    assert lbm.timer_stop() > 0.0
    assert lbm.debug_time_kernel(0, 3) > 0.0
    lbm.close()


def test_auto_keys_its_stability_bound_on_the_uploaded_state(pkg, ob):
    """`auto` takes the hand-over kernel only while alpha0 x (total density) <= 6 (csrc/bflbm.hip).  After an analytic init the
    total density is rho_hi + rho_lo of the parameters; after LBM_init(f0, g0) -- the restart path, LBM_binary.H:632-661 --
    it is whatever the upload made resident: a checkpoint of a rho_hi = 3 run loaded under HEADER DEFAULTS (alpha0 = 4,
    rho_hi = 1: 4 <= 6) has interaction strength 12 and must run an exact schedule."""
    shape = (256, 64, 64)                  # 64 tile columns x 4 chunks of 16 planes: `auto` takes the hand-over kernel here
    ob.lib().orc_set_threads(16)
    src = ob.OracleLattice(*shape, params=ob.default_params(rho_hi=3.0, alpha0=1.5))
    src.init_droplet(0.25)
    lbm = pkg.BinaryLBM(*shape)                                        # header defaults, schedule auto
    lbm.LBM_init_droplet(0.25)
    assert lbm.resolved_schedule() == "handover" and lbm.state_total_max < 0
    lbm.LBM_init(src.f, src.g)
    assert abs(lbm.state_total_max - 3.0) < 1e-12
    assert lbm.resolved_schedule() == "fused"
    lbm.LBM_timestep(3)
    ref = ob.OracleLattice(*shape)
    ref.init_from(src.f, src.g)
    for _ in range(3):
        ref.timestep()
    ob.lib().orc_set_threads(1)
    f, g = lbm.populations()
    assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g)      # exact schedule: the oracle's doubles
    # the same populations scaled to a total density of 1: inside the bound again
    lbm.LBM_init(src.f / 3.0, src.g / 3.0)
    assert abs(lbm.state_total_max - 1.0) < 1e-12 and lbm.resolved_schedule() == "handover"
    # an analytic init forgets the uploaded state
    lbm.LBM_init(src.f, src.g)
    lbm.LBM_init_stripe(0.5)
    assert lbm.state_total_max < 0 and lbm.resolved_schedule() == "handover"
    lbm.close()
    # a ring resolves every slab on the whole lattice's maximum, not on the slab's own: slab 0 holds a total density of 1
    ring = pkg.RingLBM(128, 16, 64, nslabs=4, devices=(0,))
    big = ob.OracleLattice(128, 16, 64, params=ob.default_params(rho_hi=3.0, alpha0=1.5))
    big.init_droplet(0.1)
    big.f[:, :16] /= 3.0; big.g[:, :16] /= 3.0
    ring.LBM_init(big.f, big.g)
    assert all(abs(s.state_total_max - 3.0) < 1e-12 for s in ring.slabs)
    ring.close()


def test_failed_frame_allocation_leaves_the_step_closed():
    """An explicit schedule 3 whose frames cannot be allocated fails BEFORE the step is opened: the resident state
    is intact, so the caller may switch to an exact schedule and go on, and read observables.  The allocation limit is a
    debug environment variable read once per process, hence the child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as ge
pkg = ge.load_package()
for nranks in (1, 2):
    kw = {} if nranks == 1 else dict(z0=0, z1=16, rank=0, nranks=2)
    l = pkg.BinaryLBM(128, 8, 32 if nranks == 2 else 16, schedule="handover", **kw)
    l.LBM_init_stripe(0.5)
    try:
        l.step_boundary(); l.step_interior()
        raise SystemExit("the step did not fail")
    except pkg.BflbmError as e:
        assert "frames" in str(e), str(e)
    h0 = l.LBM_hydrovars_density()                 # not 'inside an open step'
    l.set_schedule("fused")
    l.step_boundary(); l.step_interior(); l.step_finish()
    assert l.steps_done == 1
    l.close()
print("ok")
""" % root
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BFLBM_DEBUG_FRAMES_LIMIT="1"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_placement_tuning_leaves_a_fresh_context_and_the_same_doubles(pkg, ob):
    """bflbm_create draws the physical placement of the state again for slabs of at least 2^21 sites (best of 3 candidate
    allocations, timed with the context's own step kernel); bflbm_tune_placement does the same on request.  Whatever it
    keeps, the context is as freshly created and the results are the exact schedules' doubles."""
    lbm = pkg.BinaryLBM(128, 128, 128, schedule="fused")                # 2^21 sites: tuned at creation unless the environment says no
    rep = lbm.placement_report() or lbm.tune_placement(4)               # (tests/conftest.py switches the automatic tuning off to keep the suite short)
    assert rep is not None and 1 <= len(rep["candidates_ms_per_step"]) <= 8 and 0 <= rep["kept"] < len(rep["candidates_ms_per_step"])
    assert all(ms > 0 for ms in rep["candidates_ms_per_step"])
    assert rep["candidates_ms_per_step"][rep["kept"]] <= min(rep["candidates_ms_per_step"]) * 1.006
    assert lbm.steps_done == 0 and lbm.state_total_max < 0
    ob.lib().orc_set_threads(16)
    ref = ob.OracleLattice(128, 128, 128)
    ref.init_droplet(0.2)
    lbm.LBM_init_droplet(0.2)
    for _ in range(2):
        ref.timestep()
    ob.lib().orc_set_threads(1)
    lbm.LBM_timestep(2)
    f, g = lbm.populations()
    assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g)
    lbm.close()
    small = pkg.BinaryLBM(16, 16, 16)                                   # below the threshold: not tuned unless asked
    assert small.placement_report() is None
    small.LBM_init_stripe(0.5); small.LBM_timestep(3)
    rep = small.tune_placement(2)
    assert rep is not None and small.steps_done == 0
    small.LBM_init_stripe(0.5); small.LBM_timestep(3)
    r2 = ob.OracleLattice(16, 16, 16); r2.init_stripe(0.5)
    for _ in range(3):
        r2.timestep()
    f, g = small.populations()
    assert np.array_equal(f, r2.f) and np.array_equal(g, r2.g)
    small.close()
    # a slab of a decomposed lattice is tuned without its neighbours (faces not exchanged during the probe)
    slab = pkg.BinaryLBM(128, 128, 256, z0=0, z1=128, rank=0, nranks=2)
    rep = slab.placement_report() or slab.tune_placement(2)
    assert rep is not None and slab.steps_done == 0
    slab.close()
