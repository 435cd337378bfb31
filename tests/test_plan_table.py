"""The recorded plan table (tests/golden/plan_table.npz, written by tools/plan_table.py): every recorded case of
bflbm_sweep_plan_query and bflbm_fused_plan_query must return its recorded raw out[16] row.  The table was recorded before
the launch-plan layer of csrc/bflbm_fused.h was written and pins what the planner computed then; a change that is meant to
move a plan records it again.  Host arithmetic, no device."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    with np.load(os.path.join(ROOT, "tests", "golden", "plan_table.npz")) as z:
        return {k: z[k] for k in z.files}


def _rows(lib, query, cases):
    n3, out = (ctypes.c_int * 3)(), (ctypes.c_int * 16)()
    fn = getattr(lib, query)
    got = np.empty((len(cases), 16), dtype=np.int32)
    for i, case in enumerate(cases.tolist()):
        n3[:] = case[:3]
        assert fn(n3, *case[3:], out) == 0, f"{query}{tuple(case)}: {lib.bflbm_last_error().decode()}"
        got[i] = out[:]
    return got


@pytest.mark.parametrize("query", ["sweep", "fused"])
def test_every_recorded_row_is_returned_unchanged(pkg, table, query):
    cases, want = table[query + "_cases"], table[query + "_out"]
    assert len(cases) == len(want) >= 2000
    got = _rows(pkg._lib.load(), f"bflbm_{query}_plan_query", cases)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (f"{bad.size} of {len(cases)} rows moved; the first: case {cases[bad[0]].tolist()} returned "
                           f"{got[bad[0]].tolist()}, recorded {want[bad[0]].tolist()}")


def test_the_table_holds_the_shapes_the_plan_tests_name(table):
    """The recorded case list is the tool's: nothing was dropped from it by hand."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import plan_table
    sweep, fused = plan_table.case_lists()
    recorded = {tuple(c) for c in table["sweep_cases"].tolist()}
    assert recorded <= set(sweep)
    refused = [c for c in set(sweep) - recorded if c[3] == 1]              # schedule 3 is refused where handover_ok refuses
    assert not refused, refused[:5]
    assert {tuple(c) for c in table["fused_cases"].tolist()} == set(fused)
    for n in plan_table.named_shapes():
        assert (table["sweep_cases"][:, :3] == n).all(axis=1).any() and (table["fused_cases"][:, :3] == n).all(axis=1).any(), n


def test_queries_at_other_counts_do_not_move_a_concurrent_query(pkg, table):
    """Two threads alternate sweep queries at compute_units = 64 and 1024 while a third asks at 256 throughout and must
    always get the recorded row.  Before the launch-plan layer a query put its count into the global the planner read and
    put it back afterwards, so the property rested on the calls not overlapping: on the interpreter's lock, which ctypes
    gives up for the length of each call.  Now the count is an argument of the planner and the property rests on the code.
    A check that the calls can be mixed, under a scheduler that may or may not overlap them: no proof of thread safety."""
    cases, want = table["sweep_cases"], table["sweep_out"]
    rows = {cu: [i for i in np.flatnonzero((cases[:, 6] == cu) & (cases[:, 3] == 3) & (cases[:, 5] > 0))[:8]] for cu in (64, 256, 1024)}
    assert all(len(r) == 8 for r in rows.values())
    lib = pkg._lib.load()
    done, wrong = [], []

    def other(first, second):
        for k in range(300):
            for cu in (first, second):
                i = rows[cu][k % 8]
                if _rows(lib, "bflbm_sweep_plan_query", cases[i:i + 1])[0].tolist() != want[i].tolist():
                    wrong.append((cu, i))
        done.append(first)

    def steady():
        k = 0
        while len(done) < 2 or k < 300:
            i = rows[256][k % 8]
            if _rows(lib, "bflbm_sweep_plan_query", cases[i:i + 1])[0].tolist() != want[i].tolist():
                wrong.append((256, i))
            k += 1

    workers = [threading.Thread(target=other, args=(64, 1024)), threading.Thread(target=other, args=(1024, 64)),
               threading.Thread(target=steady)]
    for w in workers:
        w.start()
    for w in workers:
        w.join()
    assert not wrong, f"rows that moved: {wrong[:5]}"
