"""GPU: the full-tile unit-rate hand-over kernel carries state across march positions -- in the steady state the outputs of
fluid g wait in registers and are stored by the next position (csrc/bflbm_handover_body.inc, "deferred outputs of fluid g").
The carry begins at the first colliding position of a chunk and ends at its last one, so it is exercised here where chunks
are many and short: flat lattices with long z columns on few tiles, which the planner cuts into several chunks per column,
on one context and on two z-slabs (whose boundary-pair launches are the shortest marches there are: no steady-state position
at all), tau = 1/2, zero noise, the hand-over schedule selected explicitly (`auto` does not pick it for marches this short).

Against the CPU oracle as tests/test_gpu_handover_oracle.py does: the first step bit for bit (it pulls its ring), later steps
under tests/tolerances.py at 1e-12 and populations within 1e-13; and two contexts agree bit for bit with each other."""
import numpy as np
import pytest

import tolerances
from test_gpu_handover_oracle import _make, droplet_radius, threads   # noqa: F401  (helpers and the oracle's thread fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8, 40), (128, 8, 24), (192, 12, 16)]
STEPS = (1, 2, 12)


def _init(kind, shape):
    return ("stripe", 0.5) if kind == "stripe" else ("droplet", droplet_radius(shape))


@pytest.mark.parametrize("nslabs", [1, 2], ids=["slabs1", "slabs2"])
@pytest.mark.parametrize("kind", ["stripe", "droplet"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_short_chunks_against_the_oracle(pkg, ob, threads, shape, kind, nslabs):
    init = _init(kind, shape)
    ref = ob.OracleLattice(*shape, params=ob.default_params())
    getattr(ref, "init_" + init[0])(*init[1:])
    lbm = _make(pkg, shape, {}, nslabs)
    getattr(lbm, "LBM_init_" + init[0])(*init[1:])
    if nslabs == 1:
        assert lbm.resolved_schedule() == "handover"
    done = 0
    for steps in STEPS:
        for _ in range(steps - done):
            ref.timestep()
        lbm.LBM_timestep(steps - done)
        done = steps
        f, g = lbm.populations()
        h = lbm.LBM_hydrovars()
        what = f"{shape} {init} slabs {nslabs} step {steps}"
        if steps == 1:
            assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g), what + ": first step must be bit-exact"
            assert np.array_equal(h + 0.0, ref.h + 0.0), what
        else:
            dpop = max(np.abs(f - ref.f).max(), np.abs(g - ref.g).max())
            e = tolerances.errors(h, ref.h)
            print(what, "max |d population|", dpop, {k: e[k] for k in tolerances.MASKED})
            assert dpop < 1e-13, what
            tolerances.check(h, ref.h, what, 1e-12)
    lbm.close()


@pytest.mark.parametrize("kind", ["stripe", "droplet"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_contexts_agree_bit_for_bit(pkg, shape, kind):
    init = _init(kind, shape)
    out = []
    for _ in range(2):
        lbm = _make(pkg, shape, {}, 1)
        getattr(lbm, "LBM_init_" + init[0])(*init[1:])
        lbm.LBM_timestep(12)
        out.append(lbm.populations() + (lbm.LBM_hydrovars(),))
        lbm.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True), (shape, kind)
