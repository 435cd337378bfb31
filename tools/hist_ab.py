"""What recording histograms of the fields costs (profiles/hist_throughput.txt).

Wanted every `--every`-th step: the counts of ufx, ufy, ufz over 256 bins each, of rho and phi over 64 bins each and of
the (rho, phi) plane over 64 x 64 cells (C = 5008 counters per replica).  Three workloads:

    noisy    a 256^3 mixture at kBT = 1e-5 (tau = 1, alpha0 = 0, the mixture of the noise validation): scattered bins
    stripe   the same box as a zero-noise stripe: every velocity in one bin, the densities in runs; the contention
             worst case of adds to one LDS address
    batch    16 replicas of a 64^3 mixture with the same parameters

Three variants, one fresh process each, interleaved a / b / c `--rounds` times per workload:

    a  no observable: LBM_timestep(steps)
    b  the histogram trace: histogram_trace(every=10), LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() (of every view) plus analysis.field_histograms, every 10 steps, over --host-steps

The ranges come from the fields after a short run of the same workload (the 1 % and 99 % quantiles; +-1 around a
uniform field), before anything is timed.  The time is the host clock around the whole block, ended by a device
synchronisation (variant c is made of host round trips, so a device-side timer would miss what it costs); a warm-up
block of the same variant runs first.  Every worker process runs under its own time limit and the driver stops at the
first one that fails.

    python tools/hist_ab.py [--steps 200] [--host-steps 20] [--every 10] [--rounds 3] [--out profiles/hist_throughput.txt]
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
WORKLOADS = {"noisy": ((256, 256, 256), 1, NOISY), "stripe": ((256, 256, 256), 1, dict(kBT=0.0)), "batch": ((64, 64, 64), 16, NOISY)}
BINS = {"ufx": 256, "ufy": 256, "ufz": 256, "rho": 64, "phi": 64}
PAIRS = [("rho", "phi")]
VARIANTS = {"a": "no observable", "b": "histogram trace", "c": "hydrovs per view + numpy histograms"}


def worker(workload, variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas, params = WORKLOADS[workload]
    names = list(BINS)
    index = [pkg.plotfile.variable_names(22).index(v) for v in names]
    slots = [(names.index(a), names.index(b)) for a, b in PAIRS]
    warm = max(2 * every, steps // 20 // every * every)
    if replicas > 1:
        owner = pkg.BatchLBM(shape, params=params, replicas=replicas)
        views = owner.replicas
    else:
        owner = pkg.BinaryLBM(*shape, params=pkg.default_params(**params))
        views = [owner]
    with owner:
        for v in views:
            v.LBM_init_stripe(0.5) if workload == "stripe" else v.LBM_init_mixture()
        owner.LBM_timestep(2 * every)
        probe = views[0].LBM_hydrovars()[index]
        ranges = {}
        for k, v in enumerate(names):
            lo, hi = (float(q) for q in np.quantile(probe[k], [0.01, 0.99]))
            ranges[v] = (lo, hi, BINS[v]) if hi > lo else (lo - 1.0, lo + 1.0, BINS[v])
        del probe
        lo, hi, nb = zip(*ranges.values())
        tr = owner.histogram_trace(ranges, PAIRS, every=every, capacity=max(steps, warm) // every) if variant == "b" else None
        geometry = None if tr is None else [tr.geometry()[0]] + list(tr.geometry()[2:])      # what the library built, as observed

        def block(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    owner.LBM_timestep(every)
                    out.append([pkg.analysis.field_histograms(v.LBM_hydrovars()[index], lo, hi, nb, slots) for v in views])
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
    occupied = in_bins = None
    if counts is not None:                                 # the counters of the last sample that hold a site, replica 0
        assert (counts[-1, 0, :BINS["ufx"] + 3].sum() == sites) and counts.sum() == counts.shape[0] * replicas * 6 * sites
        occupied = int(np.count_nonzero(counts[-1, 0]))
        in_bins = float(counts[-1, 0, :BINS["ufx"]].sum()) / sites
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if counts is None else int(counts.shape[0]), occupied=occupied, in_bins=in_bins,
                          geometry=geometry, us_per_step=dt / steps * 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def drive(workload, steps, host_steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abc":
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
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    C, tile, groups, lds = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_hist_geometry: {C} counters, tiles of {tile} sites, {groups} workgroups per replica, {lds} LDS counters; "
                 f"{by['b'][0]['occupied']} counters of the last sample hold a site, {by['b'][0]['in_bins']:.3f} of the ufx sites in a bin")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds"
                 f"   a sample costs {(med['b'] - med['a']) * every:.1f} us")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-steps", type=int, default=20, help="steps of variant c, which downloads 22 fields per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--note", default=None, help="a line about the build under test for the head of the table")
    ap.add_argument("--limit", type=float, default=180.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.workload, a.worker, a.steps, a.every)
    lines = [f"# tools/hist_ab.py --steps {a.steps} --host-steps {a.host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             "# interleaved a b c; host clock around the block, ended by a device synchronisation; ufx, ufy, ufz over 256 bins, rho and",
             f"# phi over 64 bins, the (rho, phi) plane over 64 x 64 cells, wanted every {a.every}-th step; a and b over {a.steps} steps, c over {a.host_steps}"]
    if a.note:
        lines.append("# " + a.note)
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
        raise SystemExit("the histogram trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
