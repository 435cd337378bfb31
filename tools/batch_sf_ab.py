"""What structure factors of an ensemble cost (profiles/batch_sf_throughput.txt).

Workloads: batches of 64 x 32^3 and 32 x 64^3 mixtures at kBT = 1e-5, `--steps` steps, a frame of the reference's 22
pairs on hydrovs after every 10th step.  Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no structure factor: batch.LBM_timestep(steps)
    b  BatchStructFact(every=10): batch.LBM_timestep(steps), the frames are enqueued by the step call
    c  one DeviceStructFact per view, fort_structure() on each after every 10th step

The time is the host clock around the whole block, ended by a device synchronisation; a warm-up block of the same variant
runs first.  Every worker process runs under its own time limit and the driver stops at the first one that fails.

    python tools/batch_sf_ab.py [--steps 2000] [--rounds 3] [--out profiles/batch_sf_throughput.txt]
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
PARAMS = dict(alpha0=0.0, kBT=1e-5, tau_f=1.0, tau_g=1.0)
EVERY = 10
VARIANTS = {"a": "no structure factor", "b": "BatchStructFact(every=10)", "c": "DeviceStructFact per view, every 10th"}


def launches_per_frame(pkg, nrep):
    """Enqueued per frame, from the code: (b) density + observation + one transform call + accumulation for the batch;
    (c) the same four kinds per view, with one transform call per distinct variable."""
    sf = pkg.structfact
    nvar = len({v for p in zip(sf.PAIR_A, sf.PAIR_B) for v in p})
    return {"a": 0, "b": 4, "c": nrep * (3 + nvar)}


def worker(variant, n, nrep, steps):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    names = pkg.plotfile.variable_names(22)
    warm = max(2 * EVERY, steps // 20 // EVERY * EVERY)
    with pkg.BatchLBM(n, params=PARAMS, replicas=nrep) as batch:
        for rep in batch.replicas:
            rep.LBM_init_mixture()
        one = batch.structfact(names, every=EVERY) if variant == "b" else None
        per_view = [pkg.structfact.DeviceStructFact(rep, names) for rep in batch.replicas] if variant == "c" else []

        def block(k):
            if variant == "c":
                for _ in range(k // EVERY):
                    batch.LBM_timestep(EVERY)
                    for sf in per_view:
                        sf.fort_structure()
            else:
                batch.LBM_timestep(k)
            batch.sync()

        block(warm)
        t0 = time.perf_counter()
        block(steps)
        dt = time.perf_counter() - t0
        frames = one.nsamples if one else (per_view[0].nsamples if per_view else 0)
        schedule = batch.resolved_schedule()
        for sf in per_view + ([one] if one else []):
            sf.close()
    sites = n[0] * n[1] * n[2]
    print(json.dumps(dict(variant=variant, n=list(n), replicas=nrep, steps=steps, seconds=dt, schedule=schedule, frames=frames,
                          launches_per_frame=launches_per_frame(pkg, nrep)[variant],
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
    lines = [f"# tools/batch_sf_ab.py --steps {steps} --rounds {rounds}: one fresh process per variant, interleaved a b c; host clock",
             f"# around the block, ended by a device synchronisation; kBT = 1e-5 mixtures, the 22 pairs on hydrovs every {EVERY}th step"]
    for (n, nrep), by in results.items():
        lines.append(f"{n[0]}x{n[1]}x{n[2]} x {nrep} replicas, schedule {by['a'][0]['schedule']}")
        med = {}
        for v in "abc":
            us = [r["us_per_step"] for r in by[v]]
            med[v] = statistics.median(us)
            lines.append(f"  {v}  {VARIANTS[v]:<40s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   "
                         f"launches per frame {by[v][0]['launches_per_frame']:5d}   rounds: " + "  ".join(f"{u:.1f}" for u in us))
        wins = [by["b"][k]["us_per_step"] < by["c"][k]["us_per_step"] for k in range(len(by["b"]))]
        per_frame = {v: (med[v] - med["a"]) * EVERY for v in "bc"}
        lines.append(f"  per frame: b {per_frame['b']:.1f} us, c {per_frame['c']:.1f} us   b/a = {med['b'] / med['a']:.3f}   "
                     f"c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
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
            raise SystemExit("BatchStructFact was not faster than one DeviceStructFact per view in every round")


if __name__ == "__main__":
    main()
