"""What recording two-time correlations against origins kept on the device costs (profiles/lag_throughput.txt).

Wanted every `--every`-th step: the velocity autocorrelations sum_x ub_i(x, now) ub_i(x, origin), i = x, y, z, against 8
origins taken every 4th sample, and the persistence of phi about its median.  Two workloads:

    mixture  a 256^3 mixture at kBT = 1e-5 (tau = 1, alpha0 = 0, the mixture of the noise validation)
    batch    16 replicas of a 64^3 mixture with the same parameters

Four variants, one fresh process each and one process at a time, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the lag trace: lag_trace(["phi", "ubx", "uby", "ubz"], ["ubx", "uby", "ubz"], origins=8, origin_stride=4,
       persist=("phi", median), every=5), LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() (of every view) every 5 steps and analysis.lag_record of the kept frames, over
       --host-steps
    d  the yardstick: the profile trace (axis z) of the same variables and pairs, the same observation followed by a
       kernel that reads the fields of one time only

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first, long enough for
every slot of b to hold an origin.  The one read() that ends a block of b or d is inside the block and is also timed on its
own, after a synchronisation.  Variant c runs the twin, which reproduces the device's order of summation plane by plane; a
plain np.sum per origin would be faster and is not what is timed.  Every worker process runs under its own time limit and
the driver stops at the first one that fails.  No ratio is fixed beforehand: b/a is to be read against d/a of the same run.

The summing launch alone: with --launch-trace DIR the driver reads a kernel trace that was taken of the worker `s`
(rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lag_ab.py --worker s --workload W --steps N), which
takes N samples by hand on a resident state; the launches after the first origins x stride samples have every slot live.
Their median duration, apart for the samples that take an origin, against the derived bytes (8 nvars (1 + L) read per site,
8 nvars written at an origin sample, 4 for the mask) gives the bandwidth the launch achieves.

    python tools/lag_ab.py [--steps 200] [--host-steps 10] [--every 5] [--rounds 3] [--launch-trace DIR] [--out profiles/lag_throughput.txt]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOISY = dict(alpha0=0.0, kBT=1e-5, tau_f=1.0, tau_g=1.0)
WORKLOADS = {"mixture": ((256, 256, 256), 1, NOISY), "batch": ((64, 64, 64), 16, NOISY)}       # shape, replicas, parameters
VARIABLES, PAIRS, PERSIST = ["phi", "ubx", "uby", "ubz"], ["ubx", "uby", "ubz"], "phi"
ORIGINS, STRIDE = 8, 4
VARIANTS = {"a": "no observable", "b": "lag trace", "c": "hydrovs per view + numpy twin", "d": "profile trace (axis z)",
            "s": "lag trace, samples by hand"}


def worker(workload, variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas, params = WORKLOADS[workload]
    index = [pkg.plotfile.variable_names(22).index(v) for v in VARIABLES]
    slots = [(VARIABLES.index(p), VARIABLES.index(p)) for p in PAIRS]
    warm = max(ORIGINS * STRIDE * every, 2 * every) if variant == "b" else 2 * every
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
        level = float(np.median(views[0].LBM_hydrovars()[index[0]]))
        capacity = max(steps, warm) // every
        tr = None
        if variant in "bs":
            tr = owner.lag_trace(VARIABLES, PAIRS, origins=ORIGINS, origin_stride=STRIDE, persist=(PERSIST, level), every=every,
                                 capacity=(warm + steps) // every if variant == "b" else steps)
        if variant == "d":
            tr = owner.profile_trace(VARIABLES, PAIRS, axis="z", every=every, capacity=capacity)
        geometry = list(tr.geometry()) if variant in "bs" else None            # what the library built, as observed

        if variant == "s":                                 # `steps` samples by hand on the resident state: the kernel trace is the result
            for _ in range(steps):
                tr.sample()
            owner.sync()
            print(json.dumps(dict(workload=workload, variant=variant, samples=steps, geometry=geometry)), flush=True)
            return

        read_seconds = [0.0]

        def block_of(k, keep=False):
            if variant == "c":
                frames, at = [[] for _ in views], [[] for _ in views]
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    for i, v in enumerate(views):
                        frames[i].append(v.LBM_hydrovars()[index])
                        at[i].append(v.steps_done)
                return [pkg.analysis.lag_record(np.array(f), s, slots, ORIGINS, STRIDE, 0, level) for f, s in zip(frames, at)]
            owner.LBM_timestep(k)
            owner.sync()
            if tr is None:
                return None
            t_read = time.perf_counter()                   # the one read() of the block, timed apart
            rec = tr.read()
            read_seconds[0] = time.perf_counter() - t_read
            if not keep:
                tr.reset()
            return rec

        block_of(warm, keep=variant == "b")                # b keeps its record: a reset would empty the slots
        owner.sync()
        t0 = time.perf_counter()
        rec = block_of(steps)
        owner.sync()
        dt = time.perf_counter() - t0
        schedule = owner.resolved_schedule()
    sites = shape[0] * shape[1] * shape[2]
    last, samples, nbytes = None, None, None
    if variant == "b":
        steps_at, now, osteps, alive, corr = rec
        mine = steps_at[:, 0] > steps_at[-1, 0] - steps                    # the samples of the timed block
        samples, nbytes = int(mine.sum()), int(sum(v.nbytes for v in rec[1:]) * mine.sum() / len(mine))
        assert np.isfinite(now).all() and (osteps[-1] >= 0).all() and (alive[-1] >= 0).all()      # every slot live
        lags, mean, count = pkg.analysis.lag_average(steps_at[:, 0], osteps[:, 0], corr[:, 0, :, 0])
        last = [int(lags[-1]), float(mean[0] / sites), float(mean[-1] / sites), float(alive[-1, 0].min() / sites)]
    if variant == "c":
        now, osteps, alive, corr = rec[0]
        samples, nbytes = len(now), 0
        last = [int(osteps.max()), float(corr[0, 0, 0] / sites), float(np.nanmin(corr[-1, :, 0]) / sites), float(alive[-1][alive[-1] >= 0].min() / sites)]
    if variant == "d":
        samples, nbytes = int(rec[0].shape[0]), int(rec[0].nbytes)
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=samples, last=last, geometry=geometry, us_per_step=dt / steps * 1e6,
                          read_us_per_step=read_seconds[0] / steps * 1e6, record_mb=None if nbytes is None else nbytes / 1e6,
                          mlups=replicas * sites * steps / dt / 1e6)), flush=True)


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


def launch_figures(directory, workload):
    """From the kernel trace of the worker `s`: the durations of the summing launch with every slot live, in us, the samples
    that take an origin apart; None where there is no trace."""
    files = sorted(glob.glob(os.path.join(directory, workload, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        return None
    spans = []
    for r in csv.DictReader(open(files[-1])):
        name = r.get("Kernel_Name") or r.get("kernel_name") or ""
        if "k_lag_products" in name:
            spans.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    spans.sort()
    dur = [(e - s) * 1e-3 for s, e in spans]
    live = [(n, d) for n, d in enumerate(dur) if n >= ORIGINS * STRIDE]
    if not live:
        return None
    return dict(launches=len(dur), origin=[d for n, d in live if n % STRIDE == 0], plain=[d for n, d in live if n % STRIDE])


def report(workload, by, every, trace_dir):
    n, replicas = by["a"][0]["n"], by["a"][0]["replicas"]
    sites = n[0] * n[1] * n[2] * replicas
    lines = [f"{workload}: {n[0]}x{n[1]}x{n[2]} x {replicas} replica(s), schedule {by['a'][0]['schedule']}; {len(VARIABLES)} variables {VARIABLES}, "
             f"{len(PAIRS)} pairs, {ORIGINS} origins at stride {STRIDE}, persistence of {PERSIST}, every {every} steps"]
    med = {}
    for v in "abcd":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<32s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nv, npairs, r, e, words, tile, tiles, ob, mb = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_lag_geometry: {nv} variables, {npairs} pairs, {r} origins at stride {e}, {words} words per sample, tiles of {tile} sites, "
                 f"{tiles} per plane, origins {ob / 2**20:.0f} MiB, masks {mb / 2**20:.0f} MiB; largest lag, <u u>(0), <u u>(largest lag) per site and "
                 f"the smallest alive fraction of the last sample of replica 0: {by['b'][0]['last']}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    sample_b, sample_d = (med["b"] - med["a"]) * every, (med["d"] - med["a"]) * every
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   d/a = {med['d'] / med['a']:.3f}   b/d = {med['b'] / med['d']:.3f}   c/b = {med['c'] / med['b']:.2f}"
                 f"   b faster than c in {sum(wins)} of {len(wins)} rounds")
    lines.append(f"  a sample costs {sample_b:.1f} us with b and {sample_d:.1f} us with d (the observation included in both); a step costs {med['a']:.1f} us")
    rb, rd = statistics.median(x["read_us_per_step"] for x in by["b"]), statistics.median(x["read_us_per_step"] for x in by["d"])
    lines.append(f"  of which the one read() at the end of the block: b {rb:.2f} us/step for a record of {by['b'][0]['record_mb']:.3f} MB, "
                 f"d {rd:.2f} us/step for {by['d'][0]['record_mb']:.3f} MB; without it b/a = {(med['b'] - rb) / med['a']:.3f}, d/a = {(med['d'] - rd) / med['a']:.3f}")
    fig = launch_figures(trace_dir, workload) if trace_dir else None
    if fig is None:
        lines.append("  the summing launch alone: not measured yet (no kernel trace of the worker s was given)")
    else:
        plain_bytes = sites * (8 * nv * (1 + r) + 4)
        origin_bytes = sites * (8 * nv * (1 + (r - 1)) + 8 * nv + 4)       # the fresh slot is not read back, and is written
        for what, d, nbytes in (("a plain sample", fig["plain"], plain_bytes), ("a sample that takes an origin", fig["origin"], origin_bytes)):
            if d:
                m = statistics.median(d)
                lines.append(f"  the summing launch alone, {what}, every slot live: median {m:.1f} us of {len(d)} launches (min {min(d):.1f}, max {max(d):.1f}); "
                             f"derived {nbytes / 1e6:.1f} MB, {nbytes / m / 1e6:.2f} TB/s on the derived bytes")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=10, help="steps of variant c, which downloads 22 fields per replica and sample")
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--note", action="append", default=[], help="a line for the head of the table (may be given more than once)")
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one worker process in seconds")
    ap.add_argument("--launch-trace", default=None, help="directory with <workload>/ kernel traces of the worker s")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker == "s":
        return worker(a.workload, "s", a.steps, a.every)
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.workload, a.worker, a.steps, a.every)
    lines = [f"# tools/lag_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             "# interleaved a b c d; host clock around the block, ended by a device synchronisation; the autocorrelations of ubx, uby, ubz",
             f"# against {ORIGINS} origins at stride {STRIDE} and the persistence of phi, wanted every {a.every}-th step; a, b and d over {a.steps} steps, c over {a.host_steps};",
             "# b runs its timed block with every slot live; d: the profile trace (axis z) of the same variables and pairs"]
    lines += ["# " + note for note in a.note]
    ok = True
    for workload in a.workloads.split(","):
        part, wins = report(workload, drive(workload, a.steps, a.host_steps, a.every, a.rounds, a.limit), a.every, a.launch_trace)
        lines += part
        ok = ok and wins
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the lag trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
