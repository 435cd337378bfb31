"""bench.py's plain run (one timed block of exactly --steps steps), --full (what is measured beside the headline) and
--dump-outputs (a seeded sample of the state the timed steps left, for comparing two builds output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_inside_the_slab_and_small():
    import bench
    for n, z0, z1 in ((512, 0, 512), (24, 0, 24), (128, 64, 70), (8, 0, 8)):
        lo, edge = bench.dump_boxes(n, n, z0, z1)
        lo2, edge2 = bench.dump_boxes(n, n, z0, z1)
        assert np.array_equal(lo, lo2) and edge == edge2
        assert lo.shape == (bench.DUMP_BOXES, 3) and edge == (min(16, n), min(16, n), min(16, z1 - z0))
        hi = lo + np.array(edge) - 1
        assert (lo >= [0, 0, z0]).all() and (hi <= [n - 1, n - 1, z1 - 1]).all()
    lo, edge = bench.dump_boxes(512, 512, 0, 512)
    assert len({tuple(c) for c in lo}) == bench.DUMP_BOXES                  # distinct boxes over the 512^3 headline lattice
    nbytes = bench.DUMP_BOXES * int(np.prod(edge)) * (2 * 19 + 22) * 8
    assert nbytes <= 64 * 2 ** 20


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_one_block_and_dumps_what_the_oracle_computes(pkg, ob, tmp_path):
    n, warmup, steps = 24, 1, 2
    d = str(tmp_path / "out")
    r = _bench("--size", str(n), "--steps", str(steps), "--warmup", str(warmup), "--schedule", "fused", "--dump-outputs", d)
    assert r["steps"] == steps and r["config"]["schedule"] == "fused"
    assert len(r["spread"]["blocks_ms_per_step"]) == 1 and r["spread"]["blocks_ms_per_step"][0] == r["ms_per_step"] > 0
    assert r["config"]["also"] is None and "cpu_baseline" not in r
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    ref = ob.OracleLattice(n, n, n)
    ref.init_stripe(0.5)
    for _ in range(warmup + steps):
        ref.timestep()
    f, g, h, mass = (np.load(os.path.join(d, k + ".npy")) for k in ("f", "g", "hydrovars", "mass"))
    assert f.dtype == g.dtype == h.dtype == mass.dtype == np.float64
    lo, (ex, ey, ez) = __import__("bench").dump_boxes(n, n, 0, n)
    for k, (x, y, z) in enumerate(lo):
        box = (slice(None), slice(z, z + ez), slice(y, y + ey), slice(x, x + ex))
        assert np.array_equal(f[k], ref.f[box]) and np.array_equal(g[k], ref.g[box]), k   # fused: bit-exact schedule
        assert np.array_equal(h[k], ref.h[box]), k
    assert mass.tolist() == r["config"]["mass_check"]


@pytest.mark.gpu
def test_full_run_repeats_the_block_and_times_the_cpu_oracle():
    r = _bench("--size", "24", "--steps", "2", "--warmup", "1", "--full")
    assert r["steps"] == 2 and len(r["spread"]["blocks_ms_per_step"]) == 3
    assert r["cpu_baseline"]["value"] > 0
