"""What recording the shell-averaged structure factor of a coarsening mixture costs (profiles/spectrum_throughput.txt).

Workloads: a spinodal mixture (alpha0 = 2.5, kBT = 1e-5), `--steps` steps, the shell sums of S_rr, S_pp and S_rp of
hydrovsbar wanted every `--every`-th step, on
    lone    one 256^3 lattice
    batch   16 x 64^3 replicas
Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: LBM_timestep(steps)
    b  the spectrum trace: spectrum_trace(pairs, kind="shell", lb_hydrovars=True, every=20), LBM_timestep(steps), one read()
    c  through the host: LBM_hydrovars_density(ncomp=2) per lattice plus analysis.binned_spectrum per pair, every 20 steps

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant (one sample) runs first, so
the bin tables of both sides exist when the clock starts.  Every worker process runs under its own time limit and the
driver stops at the first one that fails.

    python tools/spectrum_ab.py [--workload lone batch] [--steps 400] [--every 20] [--rounds 3] [--out profiles/spectrum_throughput.txt]
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

WORKLOADS = {"lone": ((256, 256, 256), 1), "batch": ((64, 64, 64), 16)}
PARAMS = dict(alpha0=2.5, kBT=1e-5)
PAIRS = [(0, 0), (1, 1), (0, 1)]                          # rho-rho, phi-phi, rho-phi of hydrovsbar
VARIANTS = {"a": "no observable", "b": "spectrum trace", "c": "densities per lattice + numpy fftn"}


def worker(workload, variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    shape, replicas = WORKLOADS[workload]
    if replicas == 1:
        owner = pkg.BinaryLBM(*shape, params=pkg.default_params(**PARAMS))
        lattices = [owner]
    else:
        owner = pkg.BatchLBM(shape, params=PARAMS, replicas=replicas)
        lattices = owner.replicas
    for lat in lattices:
        lat.LBM_init_mixture()
    tr = owner.spectrum_trace(PAIRS, kind="shell", lb_hydrovars=True, every=every, capacity=steps // every) if variant == "b" else None
    geometry = None if tr is None else list(tr.geometry())              # what the library built, as observed

    def block(k):
        if variant == "c":
            out = []
            for _ in range(k // every):
                owner.LBM_timestep(every)
                fields = [lat.LBM_hydrovars_density(ncomp=2) for lat in lattices]
                out.append([[pkg.analysis.binned_spectrum(f[a], f[b], "shell") for a, b in PAIRS] for f in fields])
            return np.array(out)
        owner.LBM_timestep(k)
        if tr is None:
            owner.sync()
            return None
        sums = tr.read()[1]
        tr.reset()
        return sums

    block(every)
    owner.sync()
    t0 = time.perf_counter()
    sums = block(steps)
    owner.sync()
    dt = time.perf_counter() - t0
    schedule = owner.resolved_schedule()
    owner.close()
    sites = shape[0] * shape[1] * shape[2]
    print(json.dumps(dict(workload=workload, variant=variant, n=list(shape), replicas=replicas, steps=steps, every=every, seconds=dt,
                          schedule=schedule, samples=None if sums is None else int(sums.shape[0]), geometry=geometry,
                          checksum=None if sums is None else float(sums[-1, 0, 0, 1:4].sum()),
                          us_per_step=dt / steps * 1e6, mlups=replicas * sites * steps / dt / 1e6)), flush=True)


def drive(workload, steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abc":
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--workload", workload, "--steps", str(steps), "--every", str(every)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {workload} {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"{workload} round {rnd} {variant}: {rec['us_per_step']:11.1f} us/step ({rec['schedule']}, {rec['samples']} samples)", flush=True)
    return results


def report(workload, by, steps, every, rounds):
    n, replicas = WORKLOADS[workload]
    lines = [f"{n[0]}x{n[1]}x{n[2]} x {replicas} lattice(s), schedule {by['a'][0]['schedule']}, {steps} steps sampled every {every}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:11.1f} us/step   min {min(us):11.1f}  max {max(us):11.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nbins, npairs, nchunks, most = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_spectrum_geometry: {nbins} bins, {npairs} pairs, {nchunks} chunks of at most 2048 entries, at most {most} chunks in a bin")
    lines.append(f"  b  per sample over (a): {(med['b'] - med['a']) * every:.1f} us")
    lines.append(f"  last sample, bins 1..3 of S_rr: b {by['b'][0]['checksum']:.12e}   c {by['c'][0]['checksum']:.12e}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.2f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", nargs="+", choices=sorted(WORKLOADS), default=["lone", "batch"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=420.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every:
        raise SystemExit("--steps must be a multiple of --every")
    if a.worker:
        return worker(a.workload[0], a.worker, a.steps, a.every)
    lines = [] if a.append else [
        f"# tools/spectrum_ab.py --steps {a.steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant, interleaved a b c;",
        "# host clock around the block, ended by a device synchronisation; spinodal mixture alpha0 = 2.5, kBT = 1e-5; shell sums of",
        "# S_rr, S_pp, S_rp of hydrovsbar (zero_avg) wanted every 20th step"]
    ok = True
    for w in a.workload:
        results = drive(w, a.steps, a.every, a.rounds, a.limit)
        lines += report(w, results, a.steps, a.every, a.rounds)
        ok = ok and all(b["us_per_step"] < c["us_per_step"] for b, c in zip(results["b"], results["c"]))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a" if a.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the spectrum trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
