"""What recording the connected components of a field costs (profiles/cluster_throughput.txt).

Wanted every `--every`-th step: the cluster record (components, largest, sum of squared sizes, size histogram) of
{phi >= its mean} under 26-connectivity.  Three workloads:

    early      a 256^3 mixture at kBT = 1e-5, alpha0 = 2.5, right after the quench: many small components
    coarsened  the same after --coarsen-steps steps: one percolating component
    batch      16 replicas of a 64^3 mixture with the same parameters, right after the quench

Four variants, one fresh process each, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the cluster trace: cluster_trace("phi", mean, connectivity=26, every=10), LBM_timestep(steps), one read() at the end
    c  the morphology trace of the same variable and level: an existing stencil kernel over the same observed field
    d  through the host: LBM_hydrovars() (of every view) plus analysis.cluster_record, every 10 steps, over --host-steps
       (by default one sample: at 256^3 the numpy labelling alone takes a minute)

The time is the host clock around the whole block, ended by a device synchronisation; a warm-up block of the same variant
runs first (variant d: none).  Every worker process runs under its own time limit and the driver stops at the first one
that fails.  The split of a sample over its launches is not taken here: it needs a kernel trace in a run of its own.

    python tools/cluster_ab.py [--steps 200] [--host-steps 10] [--every 10] [--rounds 3] [--out profiles/cluster_throughput.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUENCH = dict(alpha0=2.5, kBT=1e-5, tau_f=1.0, tau_g=1.0)
WORKLOADS = {"early": ((256, 256, 256), 1, False), "coarsened": ((256, 256, 256), 1, True), "batch": ((64, 64, 64), 16, False)}
VARIABLE, CONNECTIVITY = "phi", 26
VARIANTS = {"a": "no observable", "b": "cluster trace", "c": "morphology trace", "d": "hydrovs per view + numpy labelling"}


def worker(workload, variant, steps, every, coarsen_steps):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas, coarsen = WORKLOADS[workload]
    index = pkg.plotfile.variable_names(22).index(VARIABLE)
    warm = max(2 * every, steps // 20 // every * every)
    if replicas > 1:
        owner = pkg.BatchLBM(shape, params=QUENCH, replicas=replicas)
        views = owner.replicas
    else:
        owner = pkg.BinaryLBM(*shape, params=pkg.default_params(**QUENCH))
        views = [owner]
    with owner:
        for v in views:
            v.LBM_init_mixture()
        owner.LBM_timestep(coarsen_steps if coarsen else 2 * every)
        level = float(views[0].LBM_hydrovars()[index].mean())
        capacity = max(steps, warm) // every
        tr = None
        if variant == "b":
            tr = owner.cluster_trace(VARIABLE, level, connectivity=CONNECTIVITY, every=every, capacity=capacity)
        if variant == "c":
            tr = owner.morphology_trace(VARIABLE, level, every=every, capacity=capacity)
        geometry = list(tr.geometry()) if variant == "b" else None            # what the library built, as observed

        def block(k):
            if variant == "d":
                out = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    out.append([pkg.analysis.cluster_record(v.LBM_hydrovars()[index], [level], "above", CONNECTIVITY) for v in views])
                return np.array(out)
            owner.LBM_timestep(k)
            if tr is None:
                owner.sync()
                return None
            rec = tr.read()[1]
            tr.reset()
            return rec

        if variant != "d":
            block(warm)
        owner.sync()
        t0 = time.perf_counter()
        rec = block(steps)
        owner.sync()
        dt = time.perf_counter() - t0
        schedule = owner.resolved_schedule()
    sites = shape[0] * shape[1] * shape[2]
    last = None
    if variant in "bd":                                    # the last sample of replica 0: ncomp, V, smax, label, sum s^2, capped
        assert rec.shape[1:] == (replicas, 1, 38) and (rec[..., 1] <= sites).all() and not rec[..., 5].any()
        last = rec[-1, 0, 0, :6].tolist()
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if rec is None else int(rec.shape[0]), last=last,
                          geometry=geometry, us_per_step=dt / steps * 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def drive(workload, a):
    results = {}
    for rnd in range(a.rounds):
        for variant in "abcd":
            k = a.host_steps if variant == "d" else a.steps
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--workload", workload, "--steps", str(k), "--every", str(a.every),
                   "--coarsen-steps", str(a.coarsen_steps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)       # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {workload} {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"{workload} round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']}, {rec['samples']} samples over {k} steps)", flush=True)
    return results


def report(workload, by, every):
    n, replicas = by["a"][0]["n"], by["a"][0]["replicas"]
    lines = [f"{workload}: {n[0]}x{n[1]}x{n[2]} x {replicas} replica(s), schedule {by['a'][0]['schedule']}"]
    med = {}
    for v in "abcd":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nl, conn, bx, by_, bz, bricks, launches = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_cluster_geometry: {nl} level(s), connectivity {conn}, bricks of {bx} x {by_} x {bz}, {bricks} per replica, {launches} launches per level; "
                 f"ncomp, V, smax, label, sum s^2, capped of the last sample of replica 0: {by['b'][0]['last']}")
    lines.append(f"  d  {by['d'][0]['samples']} sample(s) over {by['d'][0]['steps']} steps; the last of replica 0: {by['d'][0]['last']}")
    wins = [b["us_per_step"] < d["us_per_step"] for b, d in zip(by["b"], by["d"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   b/c = {med['b'] / med['c']:.3f}   d/b = {med['d'] / med['b']:.2f}   b faster than d in {sum(wins)} of {len(wins)} rounds")
    lines.append(f"  a sample costs {(med['b'] - med['a']) * every:.1f} us with b and {(med['c'] - med['a']) * every:.1f} us with c (the observation included in both)")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=10, help="steps of variant d, which downloads 22 fields and labels in numpy per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--coarsen-steps", type=int, default=2000, help="steps before the measurement of the coarsened workload")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--note", action="append", default=[], help="a line for the head of the table (may be given more than once)")
    ap.add_argument("--limit", type=float, default=600.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.workload, a.worker, a.steps, a.every, a.coarsen_steps)
    lines = [f"# tools/cluster_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds} --coarsen-steps {a.coarsen_steps}:",
             "# one fresh process per variant, interleaved a b c d; host clock around the block, ended by a device synchronisation; the components of",
             f"# phi >= its mean under {CONNECTIVITY}-connectivity, wanted every {a.every}-th step; a, b and c over {a.steps} steps, d over {a.host_steps}",
             "# (d times that many steps and its samples, not more: the numpy labelling of 256^3 sites takes about a minute per sample)"]
    lines += ["# " + note for note in a.note]
    ok = True
    for workload in a.workloads.split(","):
        part, wins = report(workload, drive(workload, a), a.every)
        lines += part
        ok = ok and wins
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the cluster trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
