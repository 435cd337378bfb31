"""What recording the chord-length distributions of a field costs (profiles/chord_throughput.txt).

Wanted every `--every`-th step: the chords along x, y and z of {phi >= level} at three levels (the quartiles of phi after
a short run of the same workload), max_length 64.  Two workloads:

    mixture  a 256^3 mixture at kBT = 1e-5 (tau = 1, alpha0 = 0, the mixture of the noise validation)
    batch    16 replicas of a 64^3 mixture with the same parameters

Four variants, one fresh process each and one process at a time, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the chord trace: chord_trace("phi", levels, max_length=64, every=10), LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() (of every view) plus analysis.chord_counts, every 10 steps, over --host-steps
    d  the yardstick: the morphology trace of the same variable and levels, an existing kernel that reads the same
       observed field once with a z march

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.  No ratio is fixed beforehand:
the only derived figure is 24 bytes per site for the three counting launches of b against about 10.5 for the one of d.

    python tools/chord_ab.py [--steps 200] [--host-steps 20] [--every 10] [--rounds 3] [--out profiles/chord_throughput.txt]
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
WORKLOADS = {"mixture": ((256, 256, 256), 1, NOISY), "batch": ((64, 64, 64), 16, NOISY)}
VARIABLE, NLEVELS, MAX_LENGTH = "phi", 3, 64
VARIANTS = {"a": "no observable", "b": "chord trace", "c": "hydrovs per view + numpy chords", "d": "morphology trace"}


def worker(workload, variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas, params = WORKLOADS[workload]
    index = pkg.plotfile.variable_names(22).index(VARIABLE)
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
        probe = views[0].LBM_hydrovars()[index]
        levels = [float(q) for q in np.quantile(probe, [0.25, 0.5, 0.75])]
        del probe
        capacity = max(steps, warm) // every
        tr = None
        if variant == "b":
            tr = owner.chord_trace(VARIABLE, levels, max_length=MAX_LENGTH, every=every, capacity=capacity)
        if variant == "d":
            tr = owner.morphology_trace(VARIABLE, levels, every=every, capacity=capacity)
        geometry = list(tr.geometry()) if variant == "b" else None            # what the library built, as observed

        def block(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    out.append([pkg.analysis.chord_counts(v.LBM_hydrovars()[index], levels, "above", MAX_LENGTH) for v in views])
                return np.array(out)
            owner.LBM_timestep(k)
            if tr is None:
                owner.sync()
                return None
            counts = tr.read()[1]
            tr.reset()
            return counts

        block(warm)
        owner.sync()
        t0 = time.perf_counter()
        counts = block(steps)
        owner.sync()
        dt = time.perf_counter() - t0
        schedule = owner.resolved_schedule()
    sites = shape[0] * shape[1] * shape[2]
    last = None
    if variant in "bc":                                    # the last sample of replica 0: V and the mean chords per level
        assert counts.shape[1:] == (replicas, NLEVELS, 1 + 3 * (3 + MAX_LENGTH)) and (counts[..., 0] <= sites).all()
        mean = pkg.analysis.chord_mean_length(counts[-1, 0], shape)
        last = [[int(counts[-1, 0, l, 0])] + [round(float(m), 3) for m in mean[l]] for l in range(NLEVELS)]
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if counts is None else int(counts.shape[0]), last=last,
                          geometry=geometry, us_per_step=dt / steps * 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


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
    lines = [f"{workload}: {n[0]}x{n[1]}x{n[2]} x {replicas} replica(s), schedule {by['a'][0]['schedule']}"]
    med = {}
    for v in "abcd":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<32s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nl, m, w, lds, gx, gy, gz = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_chord_geometry: {nl} levels, max_length {m}, {w} words per level, {lds} LDS counters per workgroup, "
                 f"{gx} / {gy} / {gz} workgroups of the x / y / z launch; V and the mean chord along x, y, z of the last sample of replica 0: {by['b'][0]['last']}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    sample_b, sample_d = (med["b"] - med["a"]) * every, (med["d"] - med["a"]) * every
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   b/d = {med['b'] / med['d']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
    lines.append(f"  a sample costs {sample_b:.1f} us with b and {sample_d:.1f} us with d (the observation included in both): "
                 f"ratio {sample_b / sample_d if sample_d > 0 else float('nan'):.3f}; the counting launches alone read 24 against about 10.5 bytes per site")
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
    lines = [f"# tools/chord_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             "# interleaved a b c d; host clock around the block, ended by a device synchronisation; the chords along x, y and z of",
             f"# phi >= its three quartiles, max_length {MAX_LENGTH}, wanted every {a.every}-th step; a, b and d over {a.steps} steps, c over {a.host_steps};",
             "# d: the morphology trace of phi at the same levels"]
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
        raise SystemExit("the chord trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
