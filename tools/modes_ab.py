"""What recording the Fourier amplitudes of a dozen wavevectors at every step costs (profiles/modes_throughput.txt).

Workload: 16 x 64^3 mixtures, alpha0 = 0, kBT = 1e-5, `--steps` steps, the six velocity components of hydrovsbar (ufx ..
ugz) wanted at every step at the 13 wavevectors of one half-space with components in {-1, 0, 1} (|m|^2 <= 3).
Three variants, one fresh process each, interleaved a / b / c `--rounds` times:

    a  no observable: LBM_timestep(steps)
    b  the mode trace: mode_trace(names, modes, lb_hydrovars=True, every=1), LBM_timestep(steps), one read()
    c  through the host: BatchLBM.LBM_hydrovars_density() plus analysis.fourier_modes, every step

The time is the host clock around the whole block, ended by a device synchronisation (variant c is made of host round
trips, so a device-side timer would miss what it costs); a warm-up block of the same variant (one sample) runs first.
Variant c takes about a second per step; `--host-steps` lets it run fewer steps than a and b, its figure is per step
either way.  Every worker process runs under its own time limit and the driver stops at the first one that fails.
The run fails when b is not faster than c in every round; no other ratio is fixed in advance.

    python tools/modes_ab.py [--steps 2000] [--host-steps 2000] [--rounds 3] [--out profiles/modes_throughput.txt]
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

SHAPE, REPLICAS = (64, 64, 64), 16
PARAMS = dict(alpha0=0.0, kBT=1e-5)
NAMES = ["ufx", "ufy", "ufz", "ugx", "ugy", "ugz"]        # of hydrovsbar
MODES = [(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1) if (z, y, x) > (0, 0, 0)]
VARIANTS = {"a": "no observable", "b": "mode trace", "c": "hydrovsbar of the batch + numpy projection"}


def worker(variant, steps):
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    modes = np.array(MODES)
    owner = pkg.BatchLBM(SHAPE, params=PARAMS, replicas=REPLICAS)
    for lat in owner.replicas:
        lat.LBM_init_mixture()
    tr = owner.mode_trace(NAMES, modes, lb_hydrovars=True, every=1, capacity=steps) if variant == "b" else None
    geometry = None if tr is None else list(tr.geometry())               # what the library built, as observed
    index = [pkg.plotfile.variable_names(9).index(v) for v in NAMES]

    def block(k):
        if variant == "c":
            out = []
            for _ in range(k):
                owner.LBM_timestep(1)
                out.append(pkg.analysis.fourier_modes(owner.LBM_hydrovars_density()[:, index], modes))
            return np.array(out)
        owner.LBM_timestep(k)
        if tr is None:
            owner.sync()
            return None
        amp = tr.read()[1]
        tr.reset()
        return amp

    block(1)
    owner.sync()
    t0 = time.perf_counter()
    amp = block(steps)
    owner.sync()
    dt = time.perf_counter() - t0
    schedule = owner.resolved_schedule()
    owner.close()
    sites = SHAPE[0] * SHAPE[1] * SHAPE[2]
    print(json.dumps(dict(variant=variant, n=list(SHAPE), replicas=REPLICAS, steps=steps, seconds=dt, schedule=schedule,
                          samples=None if amp is None else int(amp.shape[0]), geometry=geometry,
                          checksum=None if amp is None else [float(amp[0, 0, 1, 0].real), float(amp[0, 0, 1, 0].imag)],
                          us_per_step=dt / steps * 1e6, mlups=REPLICAS * sites * steps / dt / 1e6)), flush=True)


def drive(steps, host_steps, rounds, limit):
    results = {}
    for rnd in range(rounds):
        for variant in "abc":
            k = host_steps if variant == "c" else steps
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", variant, "--steps", str(k)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)     # a failure or a time limit ends the run
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"worker {variant} failed with status {r.returncode}; nothing more is started")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            results.setdefault(variant, []).append(rec)
            print(f"round {rnd} {variant}: {rec['us_per_step']:11.1f} us/step over {k} steps ({rec['schedule']}, {rec['samples']} samples)", flush=True)
    return results


def report(by, steps, host_steps):
    lines = [f"{SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]} x {REPLICAS} lattices, schedule {by['a'][0]['schedule']}, {len(NAMES)} variables x {len(MODES)} wavevectors at every step;"
             f" a and b over {steps} steps, c over {host_steps}"]
    med = {}
    for v in "abc":
        us = [r["us_per_step"] for r in by[v]]
        med[v] = statistics.median(us)
        lines.append(f"  {v}  {VARIANTS[v]:<44s} median {med[v]:11.1f} us/step   min {min(us):11.1f}  max {max(us):11.1f}   rounds: "
                     + "  ".join(f"{u:.1f}" for u in us))
    nvars, nmodes, tiles, tile = by["b"][0]["geometry"]
    lines.append(f"  b  bflbm_modes_geometry: {nvars} variables, {nmodes} wavevectors, {tiles} tiles of {tile} sites per plane")
    lines.append(f"  b  per sample over (a): {med['b'] - med['a']:.1f} us")
    lines.append(f"  first sample after the warm-up, replica 0, ufy at {MODES[0]}: b {by['b'][0]['checksum']}   c {by['c'][0]['checksum']}")
    wins = [b["us_per_step"] < c["us_per_step"] for b, c in zip(by["b"], by["c"])]
    lines.append(f"  b/a = {med['b'] / med['a']:.3f}   c/b = {med['c'] / med['b']:.1f}   b faster than c in {sum(wins)} of {len(wins)} rounds")
    return lines, all(wins)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--host-steps", type=int, default=None, help="steps of variant c (default: --steps)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=3000.0, help="time limit of one worker process in seconds")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--worker", choices=sorted(VARIANTS), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.steps)
    host_steps = a.steps if a.host_steps is None else a.host_steps
    lines = [f"# tools/modes_ab.py --steps {a.steps} --host-steps {host_steps} --rounds {a.rounds}: one fresh process per variant, interleaved a b c;",
             "# host clock around the block, ended by a device synchronisation; mixture alpha0 = 0, kBT = 1e-5; the six velocity",
             "# components of hydrovsbar at 13 wavevectors, wanted at every step"]
    results = drive(a.steps, host_steps, a.rounds, a.limit)
    table, ok = report(results, a.steps, host_steps)
    lines += table
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the mode trace was not faster than the host path in every round")


if __name__ == "__main__":
    main()
