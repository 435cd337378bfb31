"""What recording block sums of a field window costs (profiles/coarse_throughput.txt).

Wanted every `--every`-th step: the block sums of rho and phi and of the product phi * phi over a window.  Three
workloads:

    mixture  a 256^3 mixture at kBT = 1e-5 (tau = 1, alpha0 = 0, the mixture of the noise validation), the full box at
             block 4 x 4 x 4: a 64^3 coarse movie
    slice    the same lattice, one z plane at block 1 x 1 x 1: a slice
    batch    16 replicas of a 64^3 mixture with the same parameters, the full box at block 2 x 2 x 2

Four variants, one fresh process each and one process at a time, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the coarse trace: coarse_trace(["rho", "phi"], [("phi", "phi")], block, origin, extent, every=10),
       LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() (of every view) plus analysis.coarse_fields, every 10 steps, over --host-steps
    d  the yardstick: the histogram trace of the same variables (32 bins each) with the joint histogram of (rho, phi),
       the same observation followed by a different kernel (a histogram takes no pair of a variable with itself)

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  The one read()
that ends a block of b or d is inside the block and is also timed on its own, after a synchronisation: a coarse record is
a field per sample and has to cross to the host once, a histogram record is a few kilobytes.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.  No ratio is fixed beforehand:
b/a is to be read against d/a of the same run.  The only derived figures: the summing launch of b reads 8 bytes per
variable and window site (16 here) and writes 8 Q / (b_x b_y b_z); the counting launch of d reads the same 16 per site.

    python tools/coarse_ab.py [--steps 200] [--host-steps 20] [--every 10] [--rounds 3] [--out profiles/coarse_throughput.txt]
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

NOISY = dict(alpha0=0.0, kBT=1e-5, tau_f=1.0, tau_g=1.0)
# shape, replicas, parameters, (origin, extent, block)
WORKLOADS = {"mixture": ((256, 256, 256), 1, NOISY, ((0, 0, 0), (256, 256, 256), (4, 4, 4))),
             "slice": ((256, 256, 256), 1, NOISY, ((0, 0, 128), (256, 256, 1), (1, 1, 1))),
             "batch": ((64, 64, 64), 16, NOISY, ((0, 0, 0), (64, 64, 64), (2, 2, 2)))}
VARIABLES, PAIRS, HIST_PAIRS, NBINS = ["rho", "phi"], [("phi", "phi")], [("rho", "phi")], 32
VARIANTS = {"a": "no observable", "b": "coarse trace", "c": "hydrovs per view + numpy blocks", "d": "histogram trace"}


def worker(workload, variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas, params, (origin, extent, block) = WORKLOADS[workload]
    index = [pkg.plotfile.variable_names(22).index(v) for v in VARIABLES]
    slots = [(VARIABLES.index(a), VARIABLES.index(b)) for a, b in PAIRS]
    warm = max(2 * every, steps // 20 // every * every)
    if replicas > 1:
        owner = pkg.BatchLBM(shape, params=params, replicas=replicas)
        views = owner.replicas
    else:
        owner = pkg.BinaryLBM(*shape, params=pkg.default_params(**params))
        views = [owner]
    with owner:
        for v in views:
            v.LBM_init_mixture()
        owner.LBM_timestep(2 * every)
        capacity = max(steps, warm) // every
        tr = None
        if variant == "b":
            tr = owner.coarse_trace(VARIABLES, PAIRS, block=block, origin=origin, extent=extent, every=every, capacity=capacity)
        if variant == "d":
            probe = views[0].LBM_hydrovars()[index]
            ranges = {v: (float(p.min()) - 1e-3, float(p.max()) + 1e-3, NBINS) for v, p in zip(VARIABLES, probe)}
            del probe
            tr = owner.histogram_trace(ranges, HIST_PAIRS, every=every, capacity=capacity)
        geometry = list(tr.geometry()) if variant == "b" else None            # what the library built, as observed

        read_seconds = [0.0]

        def block_of(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    out.append([pkg.analysis.coarse_fields(v.LBM_hydrovars()[index], slots, origin, extent, block) for v in views])
                return np.array(out)
            owner.LBM_timestep(k)
            owner.sync()
            if tr is None:
                return None
            t_read = time.perf_counter()                   # the one read() of the block, timed apart: the record comes to the host once
            rec = tr.read()[1]
            read_seconds[0] = time.perf_counter() - t_read
            tr.reset()
            return rec

        block_of(warm)
        owner.sync()
        t0 = time.perf_counter()
        rec = block_of(steps)
        owner.sync()
        dt = time.perf_counter() - t0
        schedule = owner.resolved_schedule()
    sites = shape[0] * shape[1] * shape[2]
    last = None
    if variant in "bc":                                    # the last sample of replica 0: the mean of rho and phi and the mean block variance of phi
        cells = tuple(w // b for w, b in zip(extent[::-1], block[::-1]))
        assert rec.shape[1:] == (replicas, len(VARIABLES) + len(PAIRS)) + cells and np.isfinite(rec).all()
        m = float(block[0] * block[1] * block[2])
        var = pkg.analysis.coarse_block_variance(rec[-1, 0, 1], rec[-1, 0, 1], rec[-1, 0, 2], m)
        last = [float(rec[-1, 0, 0].mean() / m), float(rec[-1, 0, 1].mean() / m), float(var.mean())]
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if rec is None else int(rec.shape[0]), last=last,
                          geometry=geometry, us_per_step=dt / steps * 1e6, read_us_per_step=read_seconds[0] / steps * 1e6,
                          record_mb=None if rec is None else rec.nbytes / 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def drive(workload, steps, host_steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abcd":
            k = host_steps if variant == "c" else steps
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--workload", workload, "--steps", str(k), "--every", str(every)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {workload} {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"{workload} round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']}, {rec['samples']} samples over {k} steps)", flush=True)
    return results


def report(workload, by, every):
    n, replicas = by["a"][0]["n"], by["a"][0]["replicas"]
    origin, extent, block = WORKLOADS[workload][3]
    lines = [f"{workload}: {n[0]}x{n[1]}x{n[2]} x {replicas} replica(s), schedule {by['a'][0]['schedule']}; window origin {origin} extent {extent} block {block}"]
    med = {}
    for v in "abcd":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<32s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    cx, cy, cz, nq, tile, items, groups = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_coarse_geometry: {cx} x {cy} x {cz} blocks, {nq} sums, x-tile {tile} sites, {items} work items per replica, "
                 f"{groups} workgroups; mean rho, mean phi and mean block variance of phi of the last sample of replica 0: {by['b'][0]['last']}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    sample_b, sample_d = (med["b"] - med["a"]) * every, (med["d"] - med["a"]) * every
    window = extent[0] * extent[1] * extent[2]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   d/a = {med['d'] / med['a']:.3f}   b/d = {med['b'] / med['d']:.3f}   c/b = {med['c'] / med['b']:.2f}"
                 f"   b faster than c in {sum(wins)} of {len(wins)} rounds")
    lines.append(f"  a sample costs {sample_b:.1f} us with b and {sample_d:.1f} us with d (the observation included in both): "
                 f"ratio {sample_b / sample_d if sample_d > 0 else float('nan'):.3f}; the summing launch reads {8 * len(VARIABLES)} bytes per site of a window of "
                 f"{window} sites per replica, the counting launch of d {8 * len(VARIABLES)} per site of the box")
    rb, rd = statistics.median(r["read_us_per_step"] for r in by["b"]), statistics.median(r["read_us_per_step"] for r in by["d"])
    lines.append(f"  of which the one read() at the end of the block: b {rb:.1f} us/step for a record of {by['b'][0]['record_mb']:.1f} MB, "
                 f"d {rd:.1f} us/step for {by['d'][0]['record_mb']:.3f} MB; without it b/a = {(med['b'] - rb) / med['a']:.3f}, d/a = {(med['d'] - rd) / med['a']:.3f}, "
                 f"a sample {(med['b'] - rb - med['a']) * every:.1f} us with b and {(med['d'] - rd - med['a']) * every:.1f} us with d")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=20, help="steps of variant c, which downloads 22 fields per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--note", action="append", default=[], help="a line for the head of the table (may be given more than once)")
    ap.add_argument("--limit", type=float, default=180.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.workload, a.worker, a.steps, a.every)
    lines = [f"# tools/coarse_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             "# interleaved a b c d; host clock around the block, ended by a device synchronisation; the block sums of rho, phi and",
             f"# phi * phi over the workload's window, wanted every {a.every}-th step; a, b and d over {a.steps} steps, c over {a.host_steps};",
             f"# d: the histogram trace of rho and phi and of the pair (rho, phi), {NBINS} bins each"]
    lines += ["# " + note for note in a.note]
    ok = True
    for workload in a.workloads.split(","):
        part, wins = report(workload, drive(workload, a.steps, a.host_steps, a.every, a.rounds, a.limit), a.every)
        lines += part
        ok = ok and wins
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the coarse trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
