"""The plane-marching sweeps, CPU side: which launch plans the suite's hand-over and one-pass cases get
(bflbm_sweep_plan_query: the library's own planner as launch_sweep reaches it, host arithmetic, no device).

plan_chunks minimises rounds x (planes per chunk + 1); on the small lattices of tests/test_gpu_handover_oracle.py that is
always "as many chunks as possible, one round": chunks of 4 to 6 planes (pinned below: that is why
tests/test_gpu_sweep_plans.py exists), while 256^3 marches one chunk of 256 planes and 512^3 runs 8 rounds.  The table of
sweep_plan_cases.py holds the smallest lattices that reach those regimes; here each of its rows must have its plan."""
import ctypes

import pytest

import sweep_plan_cases as sp


def _query(pkg, n, schedule, **kw):
    return pkg.sweep_plan_query(n, schedule, compute_units=sp.CUS, **kw)


@pytest.mark.parametrize("regime", list(sp.HANDOVER))
def test_handover_table_has_its_plan_at_256_compute_units(pkg, regime):
    plan = _query(pkg, sp.HANDOVER[regime]["n"], "handover")
    assert plan["compute_units"] == sp.CUS
    sp.check_handover(plan, regime)
    assert plan == _query(pkg, sp.HANDOVER[regime]["n"], "handover", noise=True)     # one tile for every form of the kernel


@pytest.mark.parametrize("regime", list(sp.RING))
def test_ring_table_has_its_plan_at_256_compute_units(pkg, regime):
    plan = _query(pkg, sp.RING[regime]["n"], "handover", slab_planes=sp.SLAB_PLANES)
    sp.check_ring(plan, regime)
    assert sp.chunk_ranges(plan, first=2) == [(2, sp.SLAB_PLANES - 2)]               # between the two boundary pairs


@pytest.mark.parametrize("regime", list(sp.FUSED))
@pytest.mark.parametrize("noise", [False, True])
def test_fused_table_has_its_plan_at_256_compute_units(pkg, regime, noise):
    n = sp.FUSED[regime]["n"]
    plan = _query(pkg, n, "fused", noise=noise)
    sp.check_fused(plan, regime)
    old = pkg.fused_plan_query(n, replicas=1, noise=noise, compute_units=sp.CUS)      # the one-pass query: the same planner
    for k in ("tile_x", "tile_y", "ntx", "nty", "sx", "planes_per_chunk", "chunks", "last_chunk_planes", "workgroups", "rounds", "per_xcd", "grid"):
        assert plan[k] == old[k], (k, plan, old)


def test_fused_ring_slab_has_its_plan(pkg):
    sp.check_fused_ring(_query(pkg, sp.FUSED_RING["n"], "fused", slab_planes=sp.SLAB_PLANES))


def test_production_lattices_plan_what_the_table_stands_for(pkg):
    """The plans the table's regimes were modelled on."""
    p = _query(pkg, (256, 256, 256), "handover")
    assert sp.chunk_planes(p) == [256] and (p["workgroups"], p["rounds"]) == (256, 1)
    p = _query(pkg, (512, 512, 512), "handover")
    assert sp.chunk_planes(p) == [256, 256] and (p["ntx"], p["rounds"]) == (8, 8)
    p = _query(pkg, (320, 320, 320), "handover")
    assert sp.chunk_planes(p) == [46] * 6 + [44] and p["rounds"] == 11
    p = _query(pkg, (512, 512, 512), "handover", slab_planes=128)
    assert sp.chunk_planes(p) == [124] and p["rounds"] == 4 and (p["pair_planes"], p["pair_stride"]) == (2, 126)
    p = _query(pkg, (1024, 1024, 128), "handover", slab_planes=64)
    assert sp.chunk_planes(p) == [60] and p["rounds"] == 16


def test_existing_handover_shapes_plan_short_chunks_in_one_round(pkg):
    """The premise, as data: on every lone shape of tests/test_gpu_handover_oracle.py the hand-over kernel marches chunks
    of at most 8 planes (4 to 6 everywhere but on 250 x 250 x 8, one chunk of 8) in ONE round.  Whoever changes the
    planner sees here which regime that file covers."""
    import test_gpu_handover_oracle as ho
    longest = {}
    for n in ho.SHAPES + ho.RAGGED:
        plan = _query(pkg, n, "handover")
        lens = sp.chunk_planes(plan)
        assert sum(lens) == n[2] and min(lens) >= 1
        assert max(lens) <= 8, f"{n}: chunks {lens}"
        assert plan["rounds"] == 1 and plan["workgroups"] <= sp.CUS, f"{n}: {plan['workgroups']} workgroups in {plan['rounds']} rounds"
        longest[n] = max(lens)
    assert {n for n, l in longest.items() if l > 6} == {(250, 250, 8)}
    assert all(4 <= l <= 6 for n, l in longest.items() if n != (250, 250, 8)), longest
    plan = _query(pkg, (512, 512, 16), "handover")                       # test_bench_configuration_against_the_oracle
    assert sp.chunk_planes(plan) == [16] and plan["rounds"] == 4


def test_query_follows_the_compute_units_it_is_given(pkg):
    """compute_units replaces the device's count for the one call; 0 is the count the library holds (256 before any
    context exists, which is the case in a process without a device)."""
    n = sp.HANDOVER["cut"]["n"]
    a = pkg.sweep_plan_query(n, "handover", compute_units=256)
    b = pkg.sweep_plan_query(n, "handover", compute_units=64)
    assert a["compute_units"] == 256 and b["compute_units"] == 64
    assert b["rounds"] == -(-b["workgroups"] // 64) and b != a
    assert pkg.sweep_plan_query(n, "handover", compute_units=256) == a                 # nothing stuck from the call with 64
    held = pkg.sweep_plan_query(n, "handover")
    assert held == pkg.sweep_plan_query(n, "handover", compute_units=held["compute_units"])
    assert pkg.fused_plan_query(n, compute_units=0)["compute_units"] == held["compute_units"]
    # a slab: min_slab_rounds follows the count too (768 columns are 3 rounds of 256 but 1 of 1024: the most chunks then)
    ring = sp.RING["ring"]["n"]
    assert sp.chunk_planes(pkg.sweep_plan_query(ring, "handover", slab_planes=sp.SLAB_PLANES, compute_units=1024)) == [4, 4]


def test_a_slab_of_four_planes_is_all_boundary_pairs(pkg):
    p = _query(pkg, (128, 8, 8), "handover", slab_planes=4)
    assert (p["chunks"], p["workgroups"], p["grid"]) == (0, 0, 0) and (p["ntx"], p["nty"]) == (2, 2)
    assert (p["pair_planes"], p["pair_stride"]) == (2, 0)                              # two launches of one chunk
    p = _query(pkg, (128, 8, 10), "handover", slab_planes=5)
    assert sp.chunk_planes(p) == [1] and (p["pair_planes"], p["pair_stride"]) == (2, 3)


@pytest.mark.parametrize("n,schedule,slab,cus,pattern", [
    (None, 3, 0, 0, "null"), ((8, 0, 8), 1, 0, 0, "size"), ((128, 8, 8), 0, 0, 0, "schedule"), ((128, 8, 8), 2, 0, 0, "schedule"),
    ((16384, 16384, 8), 1, 0, 0, "32-bit"), ((128, 8, 8), 3, 0, -1, "compute_units"),
    ((128, 8, 8), 3, 3, 0, "slab_planes"), ((128, 8, 8), 3, 5, 0, "slab_planes"), ((128, 8, 8), 3, -1, 0, "slab_planes"),
    ((32, 8, 8), 3, 0, 0, "hand-over"), ((129, 8, 8), 3, 0, 0, "hand-over"), ((128, 13, 8), 3, 0, 0, "hand-over"),
])
def test_query_rejects_bad_arguments(pkg, n, schedule, slab, cus, pattern):
    lib = pkg._lib.load()
    out = (ctypes.c_int * 16)()
    n3 = (ctypes.c_int * 3)(*n) if n is not None else None
    assert lib.bflbm_sweep_plan_query(n3, schedule, 0, slab, cus, out) != 0
    msg = lib.bflbm_last_error().decode()
    assert msg.startswith("bflbm_sweep_plan_query") and pattern in msg, msg


def test_query_takes_what_the_one_pass_kernel_takes(pkg):
    """Schedule 1 has no tile restriction: the lattices schedule 3 refuses plan under it."""
    for n in ((32, 8, 8), (129, 8, 8), (128, 13, 8)):
        assert pkg.sweep_plan_query(n, "fused", compute_units=sp.CUS)["workgroups"] > 0
