"""What recording the droplet shape of an ensemble costs (profiles/shape_throughput.txt).

Workload: a batch of 64 x 32^3 droplets (radius 8, the library's default parameters with kBT = 1e-5 as in
Droplet_Fluctuation.ipynb: the droplet is stable and every ray meets its surface), `--steps` steps, the radius of the rho = 0.5 surface along the 512 rays of
analysis.ray_nodes(16, 32) from the centre of mass of the cells with rho > 0.06 wanted every `--every`-th step.  Three
variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: batch.LBM_timestep(steps)
    b  the shape trace: batch.shape_trace(every=10), batch.LBM_timestep(steps), one read() at the end
    c  through the host: LBM_hydrovars_density(ncomp=1) on every view, the centre of mass with numpy and
       analysis.droplet_radii, every 10 steps

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant runs first.  Every worker
process runs under its own time limit and the driver stops at the first one that fails.

    python tools/shape_ab.py [--steps 1000] [--every 10] [--rounds 3] [--out profiles/shape_throughput.txt]
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

SHAPE, REPLICAS = (32, 32, 32), 64
PARAMS = dict(kBT=1e-5)
RADIUS, LEVEL, THRESHOLD, STEP = 0.25, 0.5, 0.06, 0.5
VARIANTS = {"a": "no observable", "b": "shape trace", "c": "density per view + numpy rays"}


def worker(variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    warm = max(2 * every, steps // 20 // every * every)
    nodes = pkg.analysis.ray_nodes(16, 32)
    nsteps = int(min(SHAPE) / 2 / STEP)
    z, y, x = np.meshgrid(*[np.arange(m, dtype=np.float64) for m in SHAPE[::-1]], indexing="ij")
    with pkg.BatchLBM(SHAPE, params=PARAMS, replicas=REPLICAS) as batch:
        for rep in batch.replicas:
            rep.LBM_init_droplet(RADIUS)
        tr = batch.shape_trace(LEVEL, nodes, threshold=THRESHOLD, step=STEP, every=every, capacity=max(steps, warm) // every) if variant == "b" else None
        geometry = None if tr is None else list(tr.geometry())            # the launch shape the library chose, as observed

        def host_radii(rho):
            m = np.where(rho > THRESHOLD, rho, 0.0)
            centre = np.array([(m * x).sum(), (m * y).sum(), (m * z).sum()]) / m.sum()
            return pkg.analysis.droplet_radii(rho, centre, nodes[0], LEVEL, STEP, nsteps)

        def block(k):
            if variant == "c":
                out = []
                for _ in range(k // every):
                    batch.LBM_timestep(every)
                    out.append([host_radii(rep.LBM_hydrovars_density(ncomp=1)[0]) for rep in batch.replicas])
                return np.array(out)
            batch.LBM_timestep(k)
            if tr is None:
                batch.sync()
                return None
            r = tr.read()[2]
            tr.reset()
            return r

        block(warm)
        batch.sync()
        t0 = time.perf_counter()
        r = block(steps)
        batch.sync()
        dt = time.perf_counter() - t0
        schedule = batch.resolved_schedule()
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    nan = None if r is None else int(np.isnan(r).sum())                   # every ray meets the droplet's surface
    print(json.dumps(dict(variant=variant, n=list(SHAPE), replicas=REPLICAS, steps=steps, every=every, seconds=dt, schedule=schedule,
                          samples=None if r is None else int(r.shape[0]), radii_nan=nan, geometry=geometry,
                          mean_radius=None if r is None else float(np.nanmean(r)),
                          us_per_step=dt / steps * 1e6, mlups=REPLICAS * sites * steps / dt / 1e6)), flush=True)


def drive(steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abc":
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--steps", str(steps), "--every", str(every)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"round {rnd} {variant}: {rec['us_per_step']:9.1f} us/step ({rec['schedule']}, {rec['samples']} samples)", flush=True)
    return results


def report(by, steps, every, rounds):
    n = SHAPE
    lines = [f"# tools/shape_ab.py --steps {steps} --every {every} --rounds {rounds}: one fresh process per variant, interleaved a b c; host",
             "# clock around the block, ended by a device synchronisation; droplets of radius 8 with the default parameters, kBT = 1e-5,",
             f"# radii of the rho = {LEVEL} surface along the 512 rays of ray_nodes(16, 32) from the centre of mass wanted every {every}-th step",
             f"# (b)/(a) by the traffic model: 1 + (152 + 152 + 8) / (608 x {every}) = {1 + 312 / (608 * every):.3f} plus five small launches per sample",
             f"{n[0]}x{n[1]}x{n[2]} x {REPLICAS} replicas, schedule {by['a'][0]['schedule']}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<34s} median {med[v]:9.1f} us/step   min {min(us):9.1f}  max {max(us):9.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    ndir, nsteps, nseg, seg_len = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_shape_geometry: {ndir} rays of {nsteps} pairs, {nseg} segments of {seg_len} pairs (the last {nsteps - (nseg - 1) * seg_len});"
                 f" radii without a crossing: {by['b'][0]['radii_nan']} (b), {by['c'][0]['radii_nan']} (c); mean radius {by['b'][0]['mean_radius']:.3f}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=120.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every:
        raise SystemExit("--steps must be a multiple of --every")
    if a.worker:
        return worker(a.worker, a.steps, a.every)
    results = drive(a.steps, a.every, a.rounds, a.limit)
    lines = report(results, a.steps, a.every, a.rounds)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if any(r["radii_nan"] for v in "bc" for r in results[v]):
        raise SystemExit("a ray without a crossing: the droplet of this workload is meant to stay whole")
    if not all(b["us_per_step"] < c["us_per_step"] for b, c in zip(results["b"], results["c"])):
        raise SystemExit("the shape trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
