"""GPU: a context plans its launches with its own device's compute-unit count, and a plan query moves nothing a launch reads.

The launch plans (csrc/bflbm_fused.h) take the count as an argument: a context's own (read at creation), a batch's
replicas', or what a query was given.  compute_units = 0 of a query is the count of the device of the last context created.
The table of resolved schedules below was recorded from the library before the launch-plan layer existed, on a device of
256 compute units (profiles/plan_layer.txt); a device of another count fails here, it does not skip."""
import numpy as np
import pytest

import sweep_plan_cases as sp
from test_gpu_sweep_plans import BASE, _bits

pytestmark = pytest.mark.gpu

KBT = 1e-5
# what `auto` resolves to at 256 compute units: shape -> (zero noise, kBT = 1e-5)
LONE = {
    (32, 32, 32): ("two_pass", "two_pass"),
    (48, 48, 48): ("two_pass", "two_pass"),
    (64, 64, 64): ("fused", "two_pass"),
    (96, 96, 96): ("two_pass", "handover"),
    (8, 256, 64): ("two_pass", "two_pass"),
    (64, 64, 256): ("handover", "handover"),
}
BATCH = {9: ("two_pass", "two_pass"), 64: ("fused", "fused")}        # replicas of 32^3


def _device_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_table_device():
    assert _device_count() == sp.CUS, f"the device has {_device_count()} compute units; the table was recorded at {sp.CUS}"


def test_a_query_without_a_count_reports_the_device_of_the_last_context(pkg):
    n = (64, 16, 16)
    with pkg.BinaryLBM(*n):
        assert pkg.sweep_plan_query(n, "fused", compute_units=0)["compute_units"] == _device_count()
        for _ in range(3):
            assert pkg.sweep_plan_query(n, "fused", compute_units=64)["compute_units"] == 64
            assert pkg.fused_plan_query(n, replicas=4, compute_units=64)["compute_units"] == 64
        assert pkg.sweep_plan_query(n, "fused", compute_units=0)["compute_units"] == _device_count()
        assert pkg.fused_plan_query(n, compute_units=0)["compute_units"] == _device_count()


@pytest.mark.parametrize("shape", list(LONE), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
def test_auto_of_a_lattice_is_unmoved_by_an_interleaved_query(pkg, shape, noise):
    _assert_table_device()
    want = LONE[shape][int(noise)]
    with pkg.BinaryLBM(*shape, params=pkg.default_params(kBT=KBT if noise else 0.0)) as lbm:
        got = [lbm.resolved_schedule()]
        pkg.fused_plan_query(shape, replicas=1, noise=noise, compute_units=1)
        got.append(lbm.resolved_schedule())
        lbm.LBM_init_stripe(0.5)
        lbm.LBM_timestep(1)
        pkg.fused_plan_query(shape, replicas=1, noise=noise, compute_units=1)
        got.append(lbm.resolved_schedule())
    print(f"[plan owner] {shape} {'noise' if noise else 'quiet'}: {got}")
    assert got == [want] * 3


@pytest.mark.parametrize("replicas", list(BATCH))
@pytest.mark.parametrize("noise", [False, True], ids=["quiet", "noise"])
def test_auto_of_a_batch_is_unmoved_by_an_interleaved_query(pkg, replicas, noise):
    _assert_table_device()
    want = BATCH[replicas][int(noise)]
    with pkg.BatchLBM(32, params=dict(kBT=KBT if noise else 0.0), replicas=replicas) as batch:
        got = [batch.resolved_schedule()]
        pkg.fused_plan_query(32, replicas=replicas, noise=noise, compute_units=1)
        got.append(batch.resolved_schedule())
        for rep in batch.replicas:
            rep.LBM_init_stripe(0.5)
        batch.LBM_timestep(1)
        pkg.fused_plan_query(32, replicas=replicas, noise=noise, compute_units=1)
        got.append(batch.resolved_schedule())
    print(f"[plan owner] {replicas} x 32^3 {'noise' if noise else 'quiet'}: {got}")
    assert got == [want] * 3


def test_a_query_between_two_steps_leaves_the_frames_valid(pkg, ob):
    """Step 2 of the hand-over schedule reads the frames step 1 wrote only where both launches have the same plan
    (HoSig::same_geometry); otherwise it pulls the ring, computes the exact schedule's doubles and still passes parity
    (tests/test_gpu_sweep_plans.py, "step 2").  So: one step, a query at 64 compute units, one step must give the bits
    of two steps in one call on a fresh lattice, and those must differ from the exact schedule's (a frame was read)."""
    shape = (128, 16, 24)
    ref = ob.OracleLattice(*shape, params=ob.default_params(**BASE))
    ref.init_stripe(0.5)
    rng = np.random.default_rng(20240611)
    f0 = np.ascontiguousarray(ref.f * (1.0 + 0.01 * rng.standard_normal(ref.f.shape)))
    g0 = np.ascontiguousarray(ref.g * (1.0 + 0.01 * rng.standard_normal(ref.g.shape)))

    def run(schedule, calls, query):
        with pkg.BinaryLBM(*shape, params=pkg.default_params(**BASE), schedule=schedule) as lbm:
            assert lbm.resolved_schedule() == schedule
            lbm.LBM_init(f0, g0)
            for k, steps in enumerate(calls):
                if k and query:
                    assert pkg.sweep_plan_query(shape, "handover", compute_units=64)["compute_units"] == 64
                lbm.LBM_timestep(steps)
            return lbm.populations()

    f2, g2 = run("handover", (2,), False)
    f11, g11 = run("handover", (1, 1), True)
    assert not (_bits(f11) != _bits(f2)).any() and not (_bits(g11) != _bits(g2)).any(), "1 + query + 1 steps differ from 2 steps"
    fe, ge = run("fused", (2,), False)
    assert (_bits(f2) != _bits(fe)).any() or (_bits(g2) != _bits(ge)).any(), "two hand-over steps equal the exact schedule: no frame was read"
