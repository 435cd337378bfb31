"""What recording the pressure profile across the flat interfaces of an ensemble costs (profiles/profile_throughput.txt).

Workload: a batch of 16 x (8 x 256 x 64) stripes with the parameters of Flat_Interface.ipynb (alpha0 = 1.5, rho_lo = 0.1,
rho_hi = 3, kappa = 0.1, kBT = 1e-5), the plane sums along z of the pressure variables (analysis.pressure_profile_inputs:
rho, phi, af*, ag* and the four pairs rho phi, af_a ag_a) of every replica wanted every `--every`-th step.  Three
variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: batch.LBM_timestep(steps)
    b  the profile trace: batch.profile_trace(every=10), batch.LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() on every view plus analysis.plane_profiles, every 10 steps, over --host-steps

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.

    python tools/profile_ab.py [--steps 2000] [--host-steps 100] [--every 10] [--rounds 3] [--out profiles/profile_throughput.txt]
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

SHAPE, REPLICAS = (8, 256, 64), 16
PARAMS = dict(alpha0=1.5, rho_lo=0.1, rho_hi=3.0, kappa=0.1, kBT=1e-5)
VARIANTS = {"a": "no observable", "b": "profile trace", "c": "hydrovs per view + numpy plane sums"}


def worker(variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    variables, pairs = pkg.analysis.pressure_profile_inputs()
    index = [pkg.plotfile.variable_names(22).index(v) for v in variables]
    slots = [(variables.index(a), variables.index(b)) for a, b in pairs]
    warm = max(2 * every, steps // 20 // every * every)
    with pkg.BatchLBM(SHAPE, params=PARAMS, replicas=REPLICAS) as batch:
        for rep in batch.replicas:
            rep.LBM_init_stripe(0.5)
        tr = batch.profile_trace(variables, pairs, axis="z", every=every, capacity=max(steps, warm) // every) if variant == "b" else None
        geometry = None if tr is None else list(tr.geometry())            # what the library built, as observed

        def block(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    batch.LBM_timestep(every)
                    out.append([pkg.analysis.plane_profiles(rep.LBM_hydrovars()[index], slots, "z") for rep in batch.replicas])
                return np.array(out)
            batch.LBM_timestep(k)
            if tr is None:
                batch.sync()
                return None
            sums = tr.read()[0]
            tr.reset()
            return sums

        block(warm)
        batch.sync()
        t0 = time.perf_counter()
        sums = block(steps)
        batch.sync()
        dt = time.perf_counter() - t0
        schedule = batch.resolved_schedule()
    gamma = None
    if sums is not None:                                   # the last sample's mechanical surface tension, replica by replica
        means = sums[-1] / float(SHAPE[0] * SHAPE[1])
        pnt = pkg.analysis.pressure_profile(means, variables, PARAMS["alpha0"], 1.0 / 3.0, "z")[1]
        gamma = [float(g) for g in pkg.analysis.mechanical_surface_tension(pnt, interfaces=2)]
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print(json.dumps(dict(variant=variant, n=list(SHAPE), replicas=REPLICAS, steps=steps, every=every, seconds=dt, schedule=schedule,
                          samples=None if sums is None else int(sums.shape[0]), gamma=gamma, geometry=geometry,
                          us_per_step=dt / steps * 1e6, mlups=REPLICAS * sites * steps / dt / 1e6)), flush=True)


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
            print(f"round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']}, {rec['samples']} samples over {k} steps)", flush=True)
    return results


def report(by, steps, host_steps, every, rounds):
    n = SHAPE
    model = 304 + 16 + 2 * 8 * 8
    lines = [f"# tools/profile_ab.py --steps {steps} --host-steps {host_steps} --every {every} --rounds {rounds}: one fresh process per variant,",
             "# interleaved a b c; host clock around the block, ended by a device synchronisation; stripes with the Flat_Interface.ipynb",
             f"# parameters, kBT = 1e-5, plane sums along z of 8 hydrovs variables and 4 pairs wanted every {every}-th step;",
             f"# a and b over {steps} steps, c over {host_steps}",
             f"# (b)/(a) by the traffic model: 1 + {model} / (608 x {every}) = {1 + model / (608 * every):.3f} plus two small launches per sample",
             f"{n[0]}x{n[1]}x{n[2]} x {REPLICAS} replicas, schedule {by['a'][0]['schedule']}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nq, na, tile, tiles = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_profile_geometry: {nq} sums x {na} planes, tiles of {tile} sites, {tiles} per plane")
    gb, gc = by["b"][0]["gamma"], by["c"][0]["gamma"]
    lines.append(f"  gamma_mech of the last sample, mean over the replicas: b {sum(gb) / len(gb):.6f} (step {steps}), c {sum(gc) / len(gc):.6f} (step {host_steps})")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds"
                 f"   a sample costs {(med['b'] - med['a']) * every:.1f} us")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=100, help="steps of variant c, which downloads 22 fields per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every or a.host_steps % a.every:
        raise SystemExit("--steps and --host-steps must be multiples of --every")
    if a.worker:
        return worker(a.worker, a.steps, a.every)
    results = drive(a.steps, a.host_steps, a.every, a.rounds, a.limit)
    lines = report(results, a.steps, a.host_steps, a.every, a.rounds)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not all(b["us_per_step"] < c["us_per_step"] for b, c in zip(results["b"], results["c"])):
        raise SystemExit("the profile trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
