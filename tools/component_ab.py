"""What tabulating the connected components of a field costs (profiles/component_throughput.txt).

Wanted every `--every`-th step: size, origin, extent, integer moments and area of the components of {phi >= its mean}
of at least --min-size sites under 26-connectivity, --rows rows.  Two workloads:

    mixture    a 256^3 mixture at kBT = 1e-5, alpha0 = 2.5, right after the quench: many small components
    batch      16 replicas of a 64^3 mixture with the same parameters, right after the quench

Four variants, one fresh process each, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the component trace: component_trace("phi", mean, connectivity=26, ..., every=10), LBM_timestep(steps), one read()
    c  the cluster trace of the same variable, level and connectivity: the same labelling, one record per level
    d  through the host: a cluster trace's labels() (4 bytes per site) plus analysis.component_table_from_labels per
       replica, every 10 steps, over --host-steps

The time is the host clock around the whole block, ended by a device synchronisation; a warm-up block of the same variant
runs first (variant d: none).  Every worker process runs under its own time limit and the driver stops at the first one
that fails.  No ratio is asked for: the table shows b against a and c of the same session, and b against d.  The split of a
sample over its launches is not taken here: it needs a kernel trace in a run of its own.

    python tools/component_ab.py [--steps 200] [--host-steps 10] [--every 10] [--rounds 3] [--out profiles/component_throughput.txt]
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
WORKLOADS = {"mixture": ((256, 256, 256), 1), "batch": ((64, 64, 64), 16)}
VARIABLE, CONNECTIVITY = "phi", 26
VARIANTS = {"a": "no observable", "b": "component trace", "c": "cluster trace", "d": "labels() + numpy table on the host"}


def worker(workload, variant, steps, every, min_size, rows):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas = WORKLOADS[workload]
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
        owner.LBM_timestep(2 * every)
        level = float(views[0].LBM_hydrovars()[index].mean())
        capacity = max(steps, warm) // every
        tr = None
        if variant == "b":
            tr = owner.component_trace(VARIABLE, level, connectivity=CONNECTIVITY, min_size=min_size, rows=rows, every=every, capacity=capacity)
        if variant == "c":
            tr = owner.cluster_trace(VARIABLE, level, connectivity=CONNECTIVITY, every=every, capacity=capacity)
        if variant == "d":
            tr = owner.cluster_trace(VARIABLE, level, connectivity=CONNECTIVITY, every=10 ** 9, capacity=1)    # never fed: labels() only
        geometry = list(tr.geometry()) if variant == "b" else None            # what the library built, as observed

        def block(k):
            if variant == "d":
                out = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    out.append([pkg.analysis.component_table_from_labels(lab, min_size, rows)[0] for lab in tr.labels(0)])
                return np.array(out)[:, :, None, :]
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
    if variant in "bd":                                    # the header of the last sample of replica 0: ncomp, V, nqual, Vqual, nrows, capped
        assert rec.shape[1:] == (replicas, 1, 6) and (rec[..., 1] <= sites).all() and not rec[..., 5].any()
        last = rec[-1, 0, 0].tolist()
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if rec is None else int(rec.shape[0]), last=last,
                          geometry=geometry, us_per_step=dt / steps * 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def drive(workload, a):
    results = {}
    for rnd in range(a.rounds):
        for variant in "abcd":
            k = a.host_steps if variant == "d" else a.steps
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--workload", workload, "--steps", str(k), "--every", str(a.every),
                   "--min-size", str(a.min_size), "--rows", str(a.rows)]
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
    nl, conn, min_size, rows, hw, rw, launches = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_component_geometry: {nl} level(s), connectivity {conn}, min_size {min_size}, {rows} rows, {hw} + rows x {rw} words, "
                 f"{launches} launches per level; ncomp, V, nqual, Vqual, nrows, capped of the last sample of replica 0: {by['b'][0]['last']}")
    lines.append(f"  d  {by['d'][0]['samples']} sample(s) over {by['d'][0]['steps']} steps; the last header of replica 0: {by['d'][0]['last']}")
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   b/c = {med['b'] / med['c']:.3f}   d/b = {med['d'] / med['b']:.2f}")
    lines.append(f"  a sample costs {(med['b'] - med['a']) * every:.1f} us with b and {(med['c'] - med['a']) * every:.1f} us with c (the observation included in both)")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=10, help="steps of variant d, which downloads the labels and tabulates in numpy per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-size", type=int, default=8)
    ap.add_argument("--rows", type=int, default=64)
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
        return worker(a.workload, a.worker, a.steps, a.every, a.min_size, a.rows)
    lines = [f"# tools/component_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds} --min-size {a.min_size} --rows {a.rows}:",
             "# one fresh process per variant, interleaved a b c d; host clock around the block, ended by a device synchronisation; the components of",
             f"# phi >= its mean under {CONNECTIVITY}-connectivity, wanted every {a.every}-th step; a, b and c over {a.steps} steps, d over {a.host_steps}"]
    lines += ["# " + note for note in a.note]
    for workload in a.workloads.split(","):
        lines += report(workload, drive(workload, a), a.every)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
