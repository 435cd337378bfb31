#!/usr/bin/env python3
"""The recorded plan table (tests/golden/plan_table.npz): what bflbm_sweep_plan_query and bflbm_fused_plan_query return,
as raw out[16] rows, over a fixed case list.  Host arithmetic only, no device needed.  tests/test_plan_table.py replays the
recorded cases against the tree it runs in; a change of the planner that is meant to move a plan records the table again
with this tool, and the diff of the rows is what the change did.

    python tools/plan_table.py [--out tests/golden/plan_table.npz]      (BFLBM_LIB=... records another build's library)

Cases.  Every shape the plan tests name (tests/sweep_plan_cases.py, tests/batch_plan_cases.py, SHAPES and RAGGED of
tests/test_gpu_handover_oracle.py, the five production lattices of tests/test_sweep_plans.py) under every variant below, with
the slab heights and batch sizes those tests use added; and the product NX x NY x NZ under the same variants, of which every
STRIDE-th case is kept (the strides are prime to every factor of the products, so every value of every axis stays in).
    sweep query: schedule 1 and 3 (3 where the hand-over kernel takes the lattice), noise 0 and 1, slab_planes 0, 4, 5, 8,
                 nz/2 where legal (4 .. nz-4), compute_units 64, 256, 304, 1024
    fused query: replicas 1, 2, 9, 64, 256, 4096, noise 0 and 1, the same compute-unit counts
A case either query refuses is not recorded."""
import argparse
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX = (8, 16, 17, 32, 33, 64, 66, 96, 128, 250, 256, 320, 512)
NY = (4, 8, 13, 64, 250, 512)
NZ = (4, 5, 8, 13, 16, 24, 40, 64, 128, 256, 512)
CUS = (64, 256, 304, 1024)
REPLICAS = (1, 2, 9, 64, 256, 4096)
SWEEP_STRIDE, FUSED_STRIDE = 7, 5
PRODUCTION = {(256, 256, 256): 0, (512, 512, 512): 128, (320, 320, 320): 0, (1024, 1024, 128): 64}   # shape -> its slab height


def named_shapes():
    """-> {shape: (slab heights, batch sizes) the plan tests use with it}"""
    import batch_plan_cases as bp
    import sweep_plan_cases as sp
    import test_gpu_handover_oracle as ho
    named = {}

    def add(n, slab=0, replicas=1):
        s, r = named.setdefault(tuple(n), (set(), set()))
        s.add(slab)
        r.add(replicas)

    for case in list(sp.HANDOVER.values()) + list(sp.FUSED.values()):
        add(case["n"])
    for case in list(sp.RING.values()) + [sp.FUSED_RING]:
        add(case["n"], slab=sp.SLAB_PLANES)
    for family, regime in bp.CASES:
        n, replicas, _ = bp.case_shape(family, regime)
        add(n, replicas=replicas)
    for n, _ in bp.STRIP_SHAPES:
        add(n)
    for n in ho.SHAPES + ho.RAGGED + [(512, 512, 16)]:
        add(n)
    for n, slab in PRODUCTION.items():
        add(n, slab=slab)
    return named


def sweep_variants(n, slabs=()):
    slabs = sorted({s for s in (0, 4, 5, 8, n[2] // 2) + tuple(slabs) if s == 0 or 4 <= s <= n[2] - 4})
    return [n + v for v in itertools.product((1, 3), (0, 1), slabs, CUS)]


def fused_variants(n, replicas=()):
    return [n + v for v in itertools.product(sorted(set(REPLICAS + tuple(replicas))), (0, 1), CUS)]


def case_lists():
    """-> (sweep cases [nx ny nz schedule noise slab_planes compute_units], fused cases [nx ny nz replicas noise compute_units])"""
    named = named_shapes()
    sweep = [c for n, (slabs, _) in named.items() for c in sweep_variants(n, slabs)]
    fused = [c for n, (_, reps) in named.items() for c in fused_variants(n, reps)]
    lattices = [n for n in itertools.product(NX, NY, NZ) if n not in named]
    sweep += [c for n in lattices for c in sweep_variants(n)][::SWEEP_STRIDE]
    fused += [c for n in lattices for c in fused_variants(n)][::FUSED_STRIDE]
    return sweep, fused


def ask(lib, query, case):
    """The raw out[16] of one case, None where the query refuses it."""
    n3 = (ctypes.c_int * 3)(*case[:3])
    out = (ctypes.c_int * 16)()
    return None if getattr(lib, query)(n3, *[int(v) for v in case[3:]], out) else list(out)


def table(lib, query, cases):
    rows = [(c, ask(lib, query, c)) for c in cases]
    kept = [(c, r) for c, r in rows if r is not None]
    return np.array([c for c, _ in kept], dtype=np.int32), np.array([r for _, r in kept], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_table.npz"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    lib = ge.load_package()._lib.load()
    sweep, fused = case_lists()
    sc, so = table(lib, "bflbm_sweep_plan_query", sweep)
    fc, fo = table(lib, "bflbm_fused_plan_query", fused)
    np.savez_compressed(a.out, sweep_cases=sc, sweep_out=so, fused_cases=fc, fused_out=fo)
    print(f"{a.out}: {len(sc)} of {len(sweep)} sweep cases, {len(fc)} of {len(fused)} fused cases, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
