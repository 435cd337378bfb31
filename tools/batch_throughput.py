"""Replica batches against lone lattices, in one process (profiles/batch_throughput.txt).

For each shape: a lone lattice on its own `auto` schedule and on each exact schedule, then batches of B replicas on each
exact schedule and on `auto`.  Every number is the median of three timed blocks of `--steps` steps (hipEvents on the
lattice's stream) after a warm-up block; aggregate MLUPS = replicas x sites x steps / time, roofline fraction at 608 B per
site update against 8 TB/s.

    python tools/batch_throughput.py [--steps 200] [--quick]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("BFLBM_PLACEMENT_CANDIDATES", "1")      # lone lattices as small as these are never tuned anyway

import __graft_entry__ as ge  # noqa: E402

BYTES_PER_LUP = 608.0
HBM_MLUPS = 8.0e12 / BYTES_PER_LUP / 1e6                      # 13158 MLUPS at 8 TB/s

CASES = [  # (shape, batch sizes, noisy)
    ((32, 32, 32), (9, 64, 256), False),
    ((64, 64, 64), (8, 32), False),
    ((8, 256, 64), (16,), False),
    ((32, 32, 32), (9, 64, 256), True),
]
PARAMS = dict(alpha0=1.5, kappa=0.1, rho_hi=3.0)


def _time(step, timer_start, timer_stop, steps, blocks=3):
    step(max(20, steps // 10))                                  # warm-up
    out = []
    for _ in range(blocks):
        timer_start()
        step(steps)
        out.append(timer_stop())
    return statistics.median(out)


def _row(label, nrep, sites, steps, ms):
    mlups = nrep * sites * steps / (ms * 1e3)
    return f"  {label:<34s} {nrep:>4d} x  {ms / steps * 1e3:9.1f} us/step  {mlups:8.0f} MLUPS  {mlups / HBM_MLUPS:5.2f} of roofline", mlups


def run(steps, quick):
    pkg = ge.load_package()
    lines = []
    for n, sizes, noisy in CASES:
        if quick:
            sizes = sizes[:1]
        p = dict(PARAMS, kBT=1e-5 if noisy else 0.0)
        sites = n[0] * n[1] * n[2]
        lines.append(f"{n[0]}x{n[1]}x{n[2]}, kBT = {p['kBT']:g}")
        lone_best = 0.0
        for sched in ("auto", "two_pass", "fused"):
            with pkg.BinaryLBM(*n, params=pkg.default_params(**p), schedule=sched) as lone:
                lone.LBM_init_droplet(0.25)
                resolved = lone.resolved_schedule()
                ms = _time(lone.LBM_timestep, lone.timer_start, lone.timer_stop, steps)
            text, mlups = _row(f"lone, {sched} ({resolved})", 1, sites, steps, ms)
            lone_best = max(lone_best, mlups)
            lines.append(text)
        for nrep in sizes:
            for sched in ("auto", "two_pass", "fused"):
                with pkg.BatchLBM(n, params=p, replicas=nrep, schedule=sched) as b:
                    for r, rep in enumerate(b.replicas):
                        rep.LBM_init_droplet(0.2 + 0.1 * r / nrep)
                    resolved = b.resolved_schedule()
                    v = b.replicas[0]                               # its events live on the batch's stream
                    ms = _time(b.LBM_timestep, v.timer_start, v.timer_stop, steps)
                text, mlups = _row(f"batch, {sched} ({resolved})", nrep, sites, steps, ms)
                lines.append(text + f"  {mlups / lone_best:5.2f}x best lone")
        lines.append("")
        print("\n".join(lines[-1 - (3 + 3 * len(sizes)) - 1:]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block (at least 200 for the committed profile)")
    ap.add_argument("--quick", action="store_true", help="only the smallest batch of every shape")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    lines = run(a.steps, a.quick)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("# tools/batch_throughput.py --steps %d: medians of three blocks, hipEvent time on the lattice's stream\n" % a.steps)
            fh.write("# aggregate MLUPS = replicas x sites x steps / time; roofline = 608 B per site update at 8 TB/s (13158 MLUPS)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
