"""What recording the shell-averaged structure factor costs on a ring of z-slabs (profiles/ring_spectrum_throughput.txt).

Workload: a 256^3 spinodal mixture (alpha0 = 2.5, kBT = 1e-5) as a RingLBM of 4 slabs on ONE device, `--steps` steps, the
shell sums of S_rr, S_pp and S_rp of hydrovsbar wanted every `--every`-th step.  Five variants, one fresh process each,
interleaved a / b / c / d / e `--rounds` times:

    a  no observable: LBM_timestep(steps)
    b  the ring's spectrum trace: spectrum_trace(pairs, kind="shell", lb_hydrovars=True, every=20), LBM_timestep(steps), one read()
    c  through the host: RingLBM.LBM_hydrovars_density() plus analysis.binned_spectrum per pair, every 20 steps
    d  variant b with BFLBM_RING_COPY_FALLBACK=1: the transpose by strided copies instead of the gathering kernel.  The
       switch also moves the halo faces of every step by per-plane copies, so d / b mixes both;
    e  variant a with BFLBM_RING_COPY_FALLBACK=1, so that (d - e) against (b - a) is the transpose alone

The time is the host clock around the whole block, ended by a synchronisation of the ring; a warm-up block of the same
variant (one sample) runs first.  Every worker process runs under its own `timeout`, and the driver stops at the first
one that fails.  Everything is on one device: between GPUs the transpose crosses xGMI, which nothing here measures.

    python tools/ring_spectrum_ab.py [--steps 400] [--every 20] [--rounds 3] [--out profiles/ring_spectrum_throughput.txt]
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

SHAPE, NSLABS = (256, 256, 256), 4
PARAMS = dict(alpha0=2.5, kBT=1e-5)
PAIRS = [(0, 0), (1, 1), (0, 1)]                          # rho-rho, phi-phi, rho-phi of hydrovsbar
VARIANTS = {"a": "no observable", "b": "ring spectrum trace", "c": "gathered densities + numpy fftn", "d": "ring spectrum trace, copy fall-back",
            "e": "no observable, copy fall-back"}
LONE_B_OVER_A = 1.047                                     # profiles/spectrum_throughput.txt: the lone 256^3 lattice


def worker(variant, steps, every):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ring = pkg.RingLBM(*SHAPE, nslabs=NSLABS, devices=(0,), params=pkg.default_params(**PARAMS))
    ring.LBM_init_mixture()
    tr = ring.spectrum_trace(PAIRS, kind="shell", lb_hydrovars=True, every=every, capacity=steps // every) if variant in "bd" else None
    geometry = None if tr is None else list(tr.geometry())              # what the library built, as observed

    def block(k):
        if variant == "c":
            out = []
            for _ in range(k // every):
                ring.LBM_timestep(every)
                f = ring.LBM_hydrovars_density()
                out.append([[pkg.analysis.binned_spectrum(f[a], f[b], "shell") for a, b in PAIRS]])
            return np.array(out)
        ring.LBM_timestep(k)
        if tr is None:
            ring.sync()
            return None
        sums = tr.read()[1]
        tr.reset()
        return sums

    block(every)
    ring.sync()
    t0 = time.perf_counter()
    sums = block(steps)
    ring.sync()
    dt = time.perf_counter() - t0
    schedule = ring.slabs[0].resolved_schedule()
    ring.close()
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print(json.dumps(dict(variant=variant, n=list(SHAPE), nslabs=NSLABS, steps=steps, every=every, seconds=dt, schedule=schedule,
                          copy_fallback=os.environ.get("BFLBM_RING_COPY_FALLBACK", "0"),
                          samples=None if sums is None else int(sums.shape[0]), geometry=geometry,
                          checksum=None if sums is None else float(sums[-1, 0, 0, 1:4].sum()),
                          us_per_step=dt / steps * 1e6, mlups=sites * steps / dt / 1e6)), flush=True)


def drive(steps, every, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abcde":
            cmd = ["timeout", "-k", "10", str(int(limit)), sys.executable, os.path.abspath(__file__), "--worker", variant,
                   "--steps", str(steps), "--every", str(every)]
            env = dict(os.environ)
            env.pop("BFLBM_RING_COPY_FALLBACK", None)
            if variant in "de":
                env["BFLBM_RING_COPY_FALLBACK"] = "1"
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)             # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"round {rnd} {variant}: {rec['us_per_step']:11.1f} us/step ({rec['schedule']}, {rec['samples']} samples)", flush=True)
    return results


def report(by, steps, every):
    lines = [f"{SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]} as a ring of {NSLABS} slabs on one device, schedule {by['a'][0]['schedule']}, {steps} steps sampled every {every}"]
    med = {}
    for v in "abcde":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<36s} median {med[v]:11.1f} us/step   min {min(us):11.1f}  max {max(us):11.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nbins, npairs, nchunks, most = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_spectrum_geometry: {nbins} bins, {npairs} pairs, {nchunks} chunks over the slabs, at most {most} chunks in a (slab, bin)")
    per_b, per_d = (med["b"] - med["a"]) * every, (med["d"] - med["e"]) * every
    lines.append(f"  b  per sample over (a): {per_b:.1f} us      d  per sample over (e): {per_d:.1f} us")
    lines.append(f"  last sample, bins 1..3 of S_rr: b {by['b'][0]['checksum']:.12e}   c {by['c'][0]['checksum']:.12e}   d {by['d'][0]['checksum']:.12e}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f} (a lone 256^3 lattice: {LONE_B_OVER_A})   d/b = {med['d'] / med['b']:.3f} (e/a = {med['e'] / med['a']:.3f}: the halo copies of every step)   c/b = {med['c'] / med['b']:.2f}"
                 f"   b faster than c in {sum(wins)} of {len(wins)} rounds")
    if per_d <= per_b:
        lines.append("  a sample of d is not slower than one of b: on one device the gathering kernel is justified by its call count on many slabs only")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=420.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps % a.every:
        raise SystemExit("--steps must be a multiple of --every")
    if a.worker:
        return worker(a.worker, a.steps, a.every)
    lines = [
        f"# tools/ring_spectrum_ab.py --steps {a.steps} --every {a.every} --rounds {a.rounds}: one fresh process per variant, interleaved a b c d e;",
        "# host clock around the block, ended by a synchronisation of the ring; spinodal mixture alpha0 = 2.5, kBT = 1e-5; shell sums of",
        "# S_rr, S_pp, S_rp of hydrovsbar (zero_avg) wanted every 20th step.  All slabs on ONE device: between GPUs the transpose",
        "# crosses xGMI, which nothing here measures."]
    results = drive(a.steps, a.every, a.rounds, a.limit)
    lines += report(results, a.steps, a.every)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not all(b["us_per_step"] < c["us_per_step"] for b, c in zip(results["b"], results["c"])):
        raise SystemExit("the ring's spectrum trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
