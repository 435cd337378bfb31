"""What accumulating per-site noise variances on the device costs (profiles/fstat_throughput.txt).

Workload: the 256^3 noisy mixture of the per-mode variance validation (tau = 1, kBT = 1e-5, alpha0 = 0), `--steps` steps,
the per-site mean and variance over frames of the three f momentum noise modes (fn1, fn2, fn3) wanted from a frame every
`--every`-th step: NoiseCovariance.ipynb cell 3 at full size.
Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: LBM_timestep(steps)
    b  the recorder: field_stats(["fn1", "fn2", "fn3"], their three variances, source="noise", every=3),
       LBM_timestep(steps), the three cov() and mean() read once at the end
    c  through the host: thermal_noise() (38 full components) plus the same sums in numpy, every 3 steps

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant (one frame) runs first.
Variant c moves 5 GB to the host per frame; `--host-steps` lets it run fewer steps than a and b, its figure is per step
either way.  Every worker process runs under its own time limit and the driver stops at the first one that fails.
The run fails when b is not faster than c in every round; no other ratio is fixed in advance.

    python tools/fstat_ab.py [--steps 300] [--host-steps 300] [--every 3] [--rounds 3] [--out profiles/fstat_throughput.txt]
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

SHAPE = (256, 256, 256)
PARAMS = dict(alpha0=0.0, kBT=1e-5, tau_f=1.0, tau_g=1.0)
NAMES = ["fn1", "fn2", "fn3"]
VARIANTS = {"a": "no observable", "b": "field statistics", "c": "thermal_noise() + numpy sums"}


def theory():
    """kBT (2 l - l^2) / 2 with l = 1 / (tau + 1/2): the variance of a momentum noise mode (NoiseCovariance.ipynb cell 3)."""
    lam = (1.0 / PARAMS["tau_f"]) / (1.0 + 0.5 / PARAMS["tau_f"])
    return PARAMS["kBT"] * (2.0 * lam - lam ** 2) * 0.5


def worker(variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    owner = pkg.BinaryLBM(*SHAPE, params=pkg.default_params(**PARAMS))
    owner.LBM_init_mixture()
    fs = owner.field_stats(NAMES, NAMES, source="noise", every=every) if variant == "b" else None

    def block(k):
        if variant == "c":
            first = total = prod = None
            for t in range(k // every):
                owner.LBM_timestep(every)
                x = owner.thermal_noise()[0][1:4]
                if t == 0:
                    first, total, prod = x.copy(), x.copy(), np.zeros_like(x)
                else:
                    total += x
                    x -= first
                    prod += x * x
            n = k // every
            mean = total * (1.0 / n)
            return n, prod[0] * (1.0 / n) - (mean[0] - first[0]) ** 2 + mean[0] ** 2, None
        owner.LBM_timestep(k)
        owner.sync()
        if fs is None:
            return None, None, None
        t_read = time.perf_counter()
        n = fs.count
        raw = [fs.cov(v) + fs.mean(v) ** 2 for v in range(len(NAMES))]
        fs.reset()
        return n, raw[0], time.perf_counter() - t_read

    block(every)
    owner.sync()
    t0 = time.perf_counter()
    frames, raw, read_seconds = block(steps)
    owner.sync()
    dt = time.perf_counter() - t0
    schedule = owner.resolved_schedule()
    owner.close()
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print(json.dumps(dict(variant=variant, n=list(SHAPE), steps=steps, every=every, seconds=dt, schedule=schedule, samples=frames, read_seconds=read_seconds,
                          checksum=None if raw is None else float(raw.mean() / theory()),
                          us_per_step=dt / steps * 1e6, mlups=sites * steps / dt / 1e6)), flush=True)


def drive(steps, host_steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abc":
            k = host_steps if variant == "c" else steps
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--steps", str(k), "--every", str(every)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"round {rnd} {variant}: {rec['us_per_step']:11.1f} us/step over {k} steps ({rec['schedule']}, {rec['samples']} frames)", flush=True)
    return results


def report(by, steps, host_steps, every):
    lines = [f"{SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]}, schedule {by['a'][0]['schedule']}, {len(NAMES)} noise modes and their variances from a frame every {every} steps;"
             f" a and b over {steps} steps, c over {host_steps}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<32s} median {med[v]:11.1f} us/step   min {min(us):11.1f}  max {max(us):11.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    reads = statistics.median(r["read_seconds"] for r in by["b"])
    lines.append(f"  b  per frame over (a): {(med['b'] - med['a']) * every:.1f} us, of which the six reads at the end (3 cov, 3 mean, {reads * 1e3:.1f} ms"
                 f" in all) are {reads / by['b'][0]['samples'] * 1e6:.1f} us")
    lines.append(f"  site mean of <fn1^2> / theory: b {by['b'][0]['checksum']:.5f} over {by['b'][0]['samples']} frames"
                 f"   c {by['c'][0]['checksum']:.5f} over {by['c'][0]['samples']} frames")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.1f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--host-steps", type=int, default=None, help="steps of variant c (default: --steps)")
    ap.add_argument("--every", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=3000.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.steps, a.every)
    host_steps = a.steps if a.host_steps is None else a.host_steps
    lines = [f"# tools/fstat_ab.py --steps {a.steps} --host-steps {host_steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant,",
             "# interleaved a b c; host clock around the block, ended by a device synchronisation; mixture alpha0 = 0, kBT = 1e-5,",
             "# tau = 1; per-site mean and variance of the f momentum noise modes fn1, fn2, fn3"]
    results = drive(a.steps, host_steps, a.every, a.rounds, a.limit)
    table, ok = report(results, a.steps, host_steps, a.every)
    lines += table
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the recorder was not faster than the host path in every round")


if __name__ == "__main__":
    main()
