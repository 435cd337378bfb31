"""What recording the Laplace-law inputs of an ensemble of droplets costs (profiles/radial_throughput.txt).

Workload: a batch of 64 x 32^3 droplets (Surface_Tension.ipynb's box: alpha0 = 1.5, kappa = 0.1, rho_hi = 3, r = 0.25) under
thermal noise, kBT = 1e-5, the shell sums about every replica's own centre of mass of the Laplace inputs
(analysis.laplace_inputs: rho, phi, af*, ag*, the pair rho phi, the radial terms rho af . r^ and phi ag . r^; delta = 1,
28 shells) wanted every `--every`-th step.  Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: batch.LBM_timestep(steps)
    b  the radial trace: batch.radial_trace(every=10), batch.LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars() on every view, the centre of mass of the cells above the threshold and
       analysis.radial_shells in numpy, every 10 steps, over --host-steps

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.

    python tools/radial_ab.py [--steps 2000] [--host-steps 50] [--every 10] [--rounds 3] [--out profiles/radial_throughput.txt]
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

SHAPE, REPLICAS, RADIUS = (32, 32, 32), 64, 0.25
PARAMS = dict(alpha0=1.5, rho_hi=3.0, kappa=0.1, kBT=1e-5)
THRESHOLD, DELTA = 0.06, 1.0
VARIANTS = {"a": "no observable", "b": "radial trace", "c": "hydrovs per view + numpy shell sums"}


def worker(variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    an = pkg.analysis
    variables, pairs, radials = an.laplace_inputs()
    index = [pkg.plotfile.variable_names(22).index(v) for v in variables]
    ps = [(variables.index(a), variables.index(b)) for a, b in pairs]
    rd = [(variables.index(w), tuple(variables.index(c) for c in v)) for w, v in radials]
    warm = max(2 * every, steps // 20 // every * every)
    grid = np.meshgrid(*[np.arange(v, dtype=np.float64) for v in SHAPE[::-1]], indexing="ij")[::-1]      # x, y, z as [z, y, x]

    def host_sample(rep, nbins):
        x = rep.LBM_hydrovars()[index]
        w = np.where(x[0] > THRESHOLD, x[0], 0.0)
        centre = [float((w * g).sum() / w.sum()) for g in grid]
        counts, sums = an.radial_shells(x, centre, DELTA, nbins, ps, rd)
        return np.concatenate([counts[None], sums])

    with pkg.BatchLBM(SHAPE, params=PARAMS, replicas=REPLICAS) as batch:
        for rep in batch.replicas:
            rep.LBM_init_droplet(RADIUS)
        tr = None
        if variant == "b":
            tr = batch.radial_trace(variables, pairs, radials, threshold=THRESHOLD, delta=DELTA, every=every, capacity=max(steps, warm) // every)
        geometry = None if tr is None else list(tr.geometry())            # what the library built, as observed
        nbins = min(128, int(np.floor(0.5 * np.sqrt(float(sum(v * v for v in SHAPE))) / DELTA)) + 1)                 # RadialTrace's default

        def block(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    batch.LBM_timestep(every)
                    out.append([host_sample(rep, nbins) for rep in batch.replicas])
                return np.array(out)                                        # [samples, B, 1 + Q, nbins]
            batch.LBM_timestep(k)
            if tr is None:
                batch.sync()
                return None
            _, counts, sums, _ = tr.read()
            tr.reset()
            return np.concatenate([counts[:, :, None], sums], axis=2)

        block(warm)
        batch.sync()
        t0 = time.perf_counter()
        rec = block(steps)
        batch.sync()
        dt = time.perf_counter() - t0
        schedule = batch.resolved_schedule()
    dp = None
    if rec is not None:                                    # the last sample's pressure jump, replica by replica
        counts, sums = rec[-1][:, 0], rec[-1][:, 1:]
        with np.errstate(invalid="ignore", divide="ignore"):
            means = np.where(counts[:, None, :] > 0, sums / counts[:, None, :], np.nan)
        r = (np.arange(rec.shape[-1]) + 0.5) * DELTA
        dp = [float(v) for v in an.pressure_jump(an.radial_pressure(means, variables, PARAMS["alpha0"], 1.0 / 3.0), counts, r, 3.0, 16.0)]
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print(json.dumps(dict(variant=variant, n=list(SHAPE), replicas=REPLICAS, steps=steps, every=every, seconds=dt, schedule=schedule,
                          samples=None if rec is None else int(rec.shape[0]), dp=dp, geometry=geometry,
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
    lines = [f"# tools/radial_ab.py --steps {steps} --host-steps {host_steps} --every {every} --rounds {rounds}: one fresh process per variant,",
             "# interleaved a b c; host clock around the block, ended by a device synchronisation; droplets of radius 0.25 with",
             f"# alpha0 = 1.5, kappa = 0.1, rho_hi = 3, kBT = 1e-5; shell sums (delta = 1) of 8 hydrovs variables, 1 pair and 2 radial terms",
             f"# about every replica's centre of mass wanted every {every}-th step; a and b over {steps} steps, c over {host_steps}",
             f"{n[0]}x{n[1]}x{n[2]} x {REPLICAS} replicas, schedule {by['a'][0]['schedule']}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nq, nbins, tile, tiles = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_radial_geometry: {nq} sums x {nbins} shells, tiles of {tile} sites, {tiles} per plane")
    db, dc = by["b"][0]["dp"], by["c"][0]["dp"]
    lines.append(f"  Delta p of the last sample, mean over the replicas: b {sum(db) / len(db):.6f} (step {steps}), c {sum(dc) / len(dc):.6f} (step {host_steps})")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds"
                 f"   a sample costs {(med['b'] - med['a']) * every:.1f} us")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=50, help="steps of variant c, which downloads 22 fields per replica and sample")
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=150.0, help="time limit of one worker process in seconds")
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
        raise SystemExit("the radial trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
