"""What observing an ensemble every step costs (profiles/trace_throughput.txt).

Workloads: batches of 64 x 32^3 and 32 x 64^3 droplets at kBT = 1e-5, `--steps` steps, the centre of mass of every
replica wanted after every step.  Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: batch.LBM_timestep(steps)
    b  the trace: batch.trace(every=1), batch.LBM_timestep(steps), one read() at the end
    c  per lattice through the host: update_com() on every view after every step

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.

    python tools/trace_ab.py [--steps 2000] [--rounds 3] [--out profiles/trace_throughput.txt]
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

WORKLOADS = [((32, 32, 32), 64), ((64, 64, 64), 32)]
PARAMS = dict(alpha0=2.5, kBT=1e-5)
VARIANTS = {"a": "no observable", "b": "trace, every step", "c": "update_com() per view and step"}


def worker(variant, n, nrep, steps):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    warm = max(20, steps // 20)
    with pkg.BatchLBM(n, params=PARAMS, replicas=nrep) as batch:
        for r, rep in enumerate(batch.replicas):
            rep.LBM_init_droplet(0.2 + 0.1 * r / nrep)
        tr = batch.trace(every=1, capacity=max(steps, warm), threshold=0.06) if variant == "b" else None

        def block(k):
            if variant == "c":
                out = None
                for _ in range(k):
                    batch.LBM_timestep(1)
                    out = [rep.update_com() for rep in batch.replicas]
                return out
            batch.LBM_timestep(k)
            if tr is None:
                batch.sync()
                return None
            com = tr.com()
            tr.reset()
            return com

        block(warm)
        batch.sync()
        t0 = time.perf_counter()
        block(steps)
        batch.sync()
        dt = time.perf_counter() - t0
        schedule = batch.resolved_schedule()
    sites = n[0] * n[1] * n[2]
    print(json.dumps(dict(variant=variant, n=list(n), replicas=nrep, steps=steps, seconds=dt, schedule=schedule,
                          us_per_step=dt / steps * 1e6, mlups=nrep * sites * steps / dt / 1e6)), flush=True)


def drive(steps, rounds, limit):
    results = {}
    for n, nrep in WORKLOADS:
        for rnd in range(rounds):
            for variant in "abc":
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--shape", str(n[0]), "--replicas", str(nrep),
                       "--steps", str(steps)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise SystemExit(f"worker {variant} {n} x {nrep} failed with status {r.returncode}; nothing more is started")
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                results.setdefault((n, nrep), {}).setdefault(variant, []).append(rec)
                print(f"{n[0]}^3 x {nrep} round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']})", flush=True)
    return results


def report(results, steps, rounds):
    lines = [f"# tools/trace_ab.py --steps {steps} --rounds {rounds}: one fresh process per variant, interleaved a b c; host clock around",
             "# the block, ended by a device synchronisation; kBT = 1e-5, droplets (alpha0 = 2.5), centre of mass wanted after every step",
             "# (b)/(a) by the traffic model: at most 1.25 (152 B read per site against the step's 608 B) plus two small launches per step"]
    for (n, nrep), by in results.items():
        lines.append(f"{n[0]}x{n[1]}x{n[2]} x {nrep} replicas, schedule {by['a'][0]['schedule']}")
        med = {}
        for v in "abc":
            us = [r["us_per_step"] for r in by[v]]
            med[v] = statistics.median(us)
            lines.append(f"  {v}  {VARIANTS[v]:<32s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                         + "  ".join(f"{u:.1f}" for u in us))
        wins = [by["b"][k]["us_per_step"] < by["c"][k]["us_per_step"] for k in range(len(by["b"]))]
        lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
        lines.append("")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--shape", type=int, default=32, help=argparse.SUPPRESS)
    ap.add_argument("--replicas", type=int, default=64, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, (a.shape,) * 3, a.replicas, a.steps)
    results = drive(a.steps, a.rounds, a.limit)
    lines = report(results, a.steps, a.rounds)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    for by in results.values():
        if not all(b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])):
            raise SystemExit("the trace was not faster than per-view update_com() in every round")


if __name__ == "__main__":
    main()
