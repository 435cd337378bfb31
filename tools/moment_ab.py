"""What recording the box sums of all 19 kinetic moments of both fluids costs (profiles/moment_throughput.txt).

Wanted every `--every`-th step: the 95 words of a moment-trace sample (include/bflbm.h, "Moment traces").  Two workloads:

    mixture  a 256^3 mixture at kBT = 1e-5 (tau = 1, alpha0 = 0, the mixture of the noise validation)
    batch    16 replicas of a 64^3 mixture with the same parameters

Four variants, one fresh process each and one process at a time, interleaved a / b / c / d `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the moment trace: moment_trace(every=5), LBM_timestep(steps), one read() at the end
    c  through the host: populations() (of every view) every 5 steps and analysis.moment_record of them, over --host-steps
    d  the yardstick: the profile trace (axis z) of eight hydrovsbar variables, an observation into a dense intermediate
       followed by a summing kernel that reads it

With --parent-lib PATH a fifth variant p runs variant a on another build's library (BFLBM_LIB), interleaved with the rest:
the step itself must not move.  An older library lacks the bflbm_moment_* symbols, so the worker of p binds only what the
library exports; it calls nothing else.

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  The one read()
that ends a block of b or d is inside the block and is also timed on its own, after a synchronisation.  Variant c runs the
twin, which reproduces the device's order of summation plane by plane; a plain matrix product would be faster and is not
what is timed.  Every worker process runs under its own time limit and the driver stops at the first one that fails.  No
ratio is fixed beforehand.

The launches alone: the worker `s` takes `--hand-samples` samples by hand on a resident state, between two synchronisations
and under the host clock: the time of a sample's two launches (k_moment_sums and k_moment_finish), back to back on the
stream.  Against the derived bytes (304 read per site, 8 x 95 x tiles written per plane and read once more by the finishing
launch) it gives the bandwidth a sample achieves, a lower bound of the summing launch's.  With --launch-trace DIR the
driver also reads a kernel trace that was taken of the worker `s` (rocprofv3 --kernel-trace --output-format csv -d
DIR/<workload> -- python tools/moment_ab.py --worker s --workload W) for the duration of k_moment_sums alone.

    python tools/moment_ab.py [--steps 200] [--host-steps 10] [--every 5] [--rounds 3] [--parent-lib PATH] [--launch-trace DIR] [--out profiles/moment_throughput.txt]
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
BAR8 = [0, 1, 2, 3, 4, 5, 6, 7]                            # eight of the nine hydrovsbar components
STREAM_TBS = 6.3                                           # what the project quotes for a streaming kernel on this chip
VARIANTS = {"a": "no observable", "b": "moment trace", "c": "populations per view + numpy twin", "d": "profile trace, 8 hydrovsbar variables",
            "p": "no observable, the parent's library", "s": "moment trace, samples by hand"}


def worker(workload, variant, steps, every, hand_samples):
    import ctypes
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if variant == "p":                                     # another build's library: bind what it exports, call only the step
        probe = ctypes.CDLL(pkg._lib.LIB_PATH)
        pkg._lib.SIGNATURES = {k: v for k, v in pkg._lib.SIGNATURES.items() if hasattr(probe, k)}
    shape, replicas, params = WORKLOADS[workload]
    if replicas > 1:
        owner = pkg.BatchLBM(shape, params=params, replicas=replicas)
        views = owner.replicas
    else:
        owner = pkg.BinaryLBM(*shape, params=pkg.default_params(**params))
        views = [owner]
    sites = shape[0] * shape[1] * shape[2]
    with owner:
        for v in views:
            v.LBM_init_mixture()
        owner.LBM_timestep(2 * every)
        tr = None
        if variant in "bs":
            tr = owner.moment_trace(every=every, capacity=max(steps // every, hand_samples, 2))
        if variant == "d":
            tr = owner.profile_trace(BAR8, (), axis="z", source="hydrovsbar", every=every, capacity=max(steps // every, 2))
        geometry = list(tr.geometry()) if variant in "bs" else None            # what the library built, as observed

        if variant == "s":                                 # samples by hand on the resident state, between two synchronisations
            tr.sample(); tr.reset()                        # the first launch of a kernel loads its code
            owner.sync()
            t0 = time.perf_counter()
            for _ in range(hand_samples):
                tr.sample()
            owner.sync()
            dt = time.perf_counter() - t0
            print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, samples=hand_samples, geometry=geometry,
                                  us_per_sample=dt / hand_samples * 1e6)), flush=True)
            return

        read_seconds = [0.0]

        def block_of(k):
            if variant == "c":
                recs = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    recs.append([pkg.analysis.moment_record(*v.populations()) for v in views])
                return np.array(recs)
            owner.LBM_timestep(k)
            owner.sync()
            if tr is None:
                return None
            t_read = time.perf_counter()                   # the one read() of the block, timed apart
            rec = tr.read()
            read_seconds[0] = time.perf_counter() - t_read
            tr.reset()
            return rec

        block_of(every if variant == "c" else 2 * every)
        owner.sync()
        t0 = time.perf_counter()
        rec = block_of(steps)
        owner.sync()
        dt = time.perf_counter() - t0
        schedule = owner.resolved_schedule()
    last, samples, nbytes = None, None, None
    if variant in "bc":
        sums = rec[1] if variant == "b" else rec
        samples, nbytes = int(sums.shape[0]), int(sums.nbytes) if variant == "b" else 0
        assert np.isfinite(sums).all()
        e = pkg.analysis.equipartition(sums[-1, 0], sites)[2]
        last = [float(sums[-1, 0, 0] / sites), float(sums[-1, 0, 19] / sites), float(e[4:10].mean()), float(e[10:].mean())]
    if variant == "d":
        samples, nbytes = int(rec[0].shape[0]), int(rec[0].nbytes)
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=samples, last=last, geometry=geometry, us_per_step=dt / steps * 1e6,
                          read_us_per_step=read_seconds[0] / steps * 1e6, record_mb=None if nbytes is None else nbytes / 1e6,
                          mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def run_worker(workload, variant, args, limit, parent_lib=None):
    env = dict(os.environ)
    if variant == "p":
        env["BFLBM_LIB"] = parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--workload", workload] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)     # a failure or a time limit ends the run
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"worker {workload} {variant} failed with status {r.returncode}; nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def drive(workload, a):
    results = {}
    order = "apbcd" if a.parent_lib else "abcd"
    for rnd in range(a.rounds):
        for variant in order:
            k = a.host_steps if variant == "c" else a.steps
            rec = run_worker(workload, variant, ["--steps", str(k), "--every", str(a.every)], a.limit, a.parent_lib)
            results.setdefault(variant, []).append(rec)
            print(f"{workload} round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']}, {rec['samples']} samples over {k} steps)", flush=True)
    results["s"] = [run_worker(workload, "s", ["--hand-samples", str(a.hand_samples), "--every", str(a.every)], a.limit)]
    print(f"{workload} s: {results['s'][0]['us_per_sample']:9.1f} us per sample by hand", flush=True)
    return results


def launch_figures(directory, workload):
    """From the kernel trace of the worker `s`: the durations of k_moment_sums in us, the first (which loads the code) left
    out; None where there is no trace."""
    files = sorted(glob.glob(os.path.join(directory, workload, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        return None
    spans = []
    for r in csv.DictReader(open(files[-1])):
        name = r.get("Kernel_Name") or r.get("kernel_name") or ""
        if "k_moment_sums" in name:
            spans.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    spans.sort()
    return [(e - s) * 1e-3 for s, e in spans][1:] or None


def report(workload, by, every, trace_dir):
    n, replicas = by["a"][0]["n"], by["a"][0]["replicas"]
    sites = n[0] * n[1] * n[2] * replicas
    lines = [f"{workload}: {n[0]}x{n[1]}x{n[2]} x {replicas} replica(s), schedule {by['a'][0]['schedule']}; 95 words per replica and sample, every {every} steps"]
    med = {}
    for v in [v for v in "apbcd" if v in by]:
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<40s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    words, tile, tiles = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_moment_geometry: {words} words per sample, tiles of {tile} sites, {tiles} per plane; rho_f, rho_g per site and the mean "
                 f"equipartition ratio of the total fluid's stress and ghost modes in the last sample of replica 0: {by['b'][0]['last']}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    sample_b, sample_d = (med["b"] - med["a"]) * every, (med["d"] - med["a"]) * every
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   d/a = {med['d'] / med['a']:.3f}   b/d = {med['b'] / med['d']:.3f}   c/b = {med['c'] / med['b']:.2f}"
                 f"   b faster than c in {sum(wins)} of {len(wins)} rounds")
    lines.append(f"  a sample costs {sample_b:.1f} us with b and {sample_d:.1f} us with d (its observation included); a step costs {med['a']:.1f} us")
    if "p" in by:
        us_a, us_p = [r["us_per_step"] for r in by["a"]], [r["us_per_step"] for r in by["p"]]
        inside = min(us_p) <= med["a"] <= max(us_p) or min(us_a) <= med["p"] <= max(us_a)
        lines.append(f"  the step itself: a {med['a']:.1f} us/step (rounds {min(us_a):.1f} .. {max(us_a):.1f}) against the parent's library p {med['p']:.1f} "
                     f"({min(us_p):.1f} .. {max(us_p):.1f}): a/p = {med['a'] / med['p']:.4f}, "
                     + ("within the spread of the rounds" if inside else "OUTSIDE the spread of the rounds"))
    rb, rd = statistics.median(x["read_us_per_step"] for x in by["b"]), statistics.median(x["read_us_per_step"] for x in by["d"])
    lines.append(f"  of which the one read() at the end of the block: b {rb:.2f} us/step for a record of {by['b'][0]['record_mb']:.3f} MB, "
                 f"d {rd:.2f} us/step for {by['d'][0]['record_mb']:.3f} MB")
    planes = n[2] * replicas
    nbytes = sites * 304 + 2 * planes * 95 * tiles * 8     # the populations once; the partials written and read once
    s = by["s"][0]
    lines.append(f"  a sample by hand (k_moment_sums + k_moment_finish back to back, host clock over {s['samples']} samples between two synchronisations): "
                 f"{s['us_per_sample']:.1f} us; derived {nbytes / 1e6:.1f} MB, {nbytes / s['us_per_sample'] / 1e6:.2f} TB/s on the derived bytes, "
                 f"{nbytes / s['us_per_sample'] / 1e6 / STREAM_TBS:.2f} of the {STREAM_TBS} TB/s of a streaming kernel")
    dur = launch_figures(trace_dir, workload) if trace_dir else None
    if dur is None:
        lines.append("  k_moment_sums alone: no kernel trace of the worker s was given; the figure above includes the finishing launch and the launch gaps")
    else:
        m = statistics.median(dur)
        lines.append(f"  k_moment_sums alone, from a kernel trace: median {m:.1f} us of {len(dur)} launches (min {min(dur):.1f}, max {max(dur):.1f}); "
                     f"derived {sites * 304 / 1e6:.1f} MB read, {sites * 304 / m / 1e6:.2f} TB/s, {sites * 304 / m / 1e6 / STREAM_TBS:.2f} of {STREAM_TBS} TB/s")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=10, help="steps of variant c, which downloads 38 populations per site, replica and sample")
    ap.add_argument("--every", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hand-samples", type=int, default=40, help="samples the worker s takes by hand")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--parent-lib", default=None, help="another build's libbflbm.so: variant p, the bare step on it")
    ap.add_argument("--note", action="append", default=[], help="a line for the head of the table (may be given more than once)")
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one worker process in seconds")
    ap.add_argument("--launch-trace", default=None, help="directory with <workload>/ kernel traces of the worker s")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker == "s":
        return worker(a.workload, "s", a.steps, a.every, a.hand_samples)
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.workload, a.worker, a.steps, a.every, a.hand_samples)
    lines = [f"# tools/moment_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             f"# interleaved {' '.join('apbcd' if a.parent_lib else 'abcd')}; host clock around the block, ended by a device synchronisation; the 95 box sums of the kinetic",
             f"# moments of both fluids, wanted every {a.every}-th step; a, b, d{' and p' if a.parent_lib else ''} over {a.steps} steps, c over {a.host_steps};",
             "# d: the profile trace (axis z) of eight hydrovsbar variables"]
    lines += ["# " + note for note in a.note]
    ok = True
    for workload in a.workloads.split(","):
        part, wins = report(workload, drive(workload, a), a.every, a.launch_trace)
        lines += part
        ok = ok and wins
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the moment trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
