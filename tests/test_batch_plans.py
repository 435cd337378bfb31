"""Replica batches, CPU side: which launch plans the suite's batch cases get (bflbm_fused_plan_query: the library's own
planner, host arithmetic, no device).

plan_chunks minimises rounds x (planes per chunk + 1); while the whole launch has fewer than `compute units` workgroups
the cheapest plan is the one with the most chunks.  At 256 compute units every batch the other test files run therefore
marches chunks of 2 planes on the narrow tiles (pinned below: that is why tests/test_gpu_batch_plans.py exists), while the
batch sizes the README quotes run one or two long chunks per column.  The table of batch_plan_cases.py puts every tile
family under long, ragged, one-plane-tail and exactly-full plans; here each of its cases must have its properties."""
import ctypes

import pytest

import batch_plan_cases as bp


def _query(pkg, n, replicas, noise):
    return pkg.fused_plan_query(n, replicas=replicas, noise=noise, compute_units=bp.CUS)


@pytest.mark.parametrize("family,regime", bp.CASES)
def test_case_table_has_its_plan_at_256_compute_units(pkg, family, regime):
    n, replicas, noise = bp.case_shape(family, regime)
    plan = _query(pkg, n, replicas, noise)
    assert plan["compute_units"] == bp.CUS
    bp.check_case(plan, family, regime)


@pytest.mark.parametrize("n,ntx", bp.STRIP_SHAPES)
@pytest.mark.parametrize("replicas", [1, 3])
def test_strip_shapes_have_a_narrower_last_strip(pkg, n, ntx, replicas):
    bp.check_strips(_query(pkg, n, replicas, False), n, ntx)


# what the batches of the other test files plan: (n, replicas, noise) -> tile, planes of every chunk, workgroups
EXISTING = [
    ("batch parity 5 x 32^3 quiet", (32, 32, 32), 5, False, (32, 16), [2] * 16, 160),
    ("batch parity 4 x 40x24x20 quiet", (40, 24, 20), 4, False, (64, 8), [2] * 10, 120),
    ("batch parity 4 x 8x256x64 quiet", (8, 256, 64), 4, False, (8, 64), [4] * 16, 256),
    ("batch parity 3 x 64^3 quiet", (64, 64, 64), 3, False, (64, 8), [7] * 9 + [1], 240),
    ("batch noise 3 x 32^3", (32, 32, 32), 3, True, (32, 8), [2] * 16, 192),
    ("trace noise batch 5 x 24^3", (24, 24, 24), 5, True, (32, 8), [2] * 12, 180),
    ("iface noise batch 3 x 20x28x24", (20, 28, 24), 3, True, (32, 8), [2] * 12, 144),
]


@pytest.mark.parametrize("what,n,replicas,noise,tile,chunks,workgroups", EXISTING)
def test_existing_batch_cases_plan_short_chunks(pkg, what, n, replicas, noise, tile, chunks, workgroups):
    """The pin that records why the plan cases exist: one round, and on every narrow tile (width < 64, batch noise tile
    included) chunks of 2 planes -- four march positions, the four-slot density ring never wraps -- or 4."""
    plan = _query(pkg, n, replicas, noise)
    assert (plan["tile_x"], plan["tile_y"]) == tile, what
    assert bp.chunk_planes(plan, n[2]) == chunks, what
    assert plan["workgroups"] == workgroups and plan["rounds"] == 1, what
    assert plan["ntx"] == 1, what                                       # never two tiles wide
    if tile[0] < 64:
        assert max(chunks) <= 4, what


@pytest.mark.parametrize("nx", [8, 16, 24, 32])
def test_lone_narrow_lattices_plan_chunks_of_two_planes(pkg, nx):
    """A lone lattice with nx <= 32 is at most 128 workgroups: always the most chunks."""
    plan = _query(pkg, (nx, 32, 32), 1, False)
    assert plan["tile_x"] == max(8, min(32, 1 << (nx - 1).bit_length())) and plan["workgroups"] <= 128
    assert bp.chunk_planes(plan, 32) == [2] * 16


ADVERTISED = [
    ("64 x 32^3 quiet", (32, 32, 32), 64, False, (32, 16), [16, 16], 256, 1),
    ("64 x 32^3 noise", (32, 32, 32), 64, True, (32, 8), [32], 256, 1),
    ("32 x 64^3 noise", (64, 64, 64), 32, True, (32, 8), [64], 512, 2),
]


@pytest.mark.parametrize("what,n,replicas,noise,tile,chunks,workgroups,rounds", ADVERTISED)
def test_advertised_batches_plan_long_chunks(pkg, what, n, replicas, noise, tile, chunks, workgroups, rounds):
    plan = _query(pkg, n, replicas, noise)
    assert (plan["tile_x"], plan["tile_y"]) == tile, what
    assert bp.chunk_planes(plan, n[2]) == chunks, what
    assert (plan["workgroups"], plan["rounds"]) == (workgroups, rounds), what
    assert plan["ntx"] == (2 if n[0] == 64 and noise else 1), what      # the 64-wide noise batch: two tiles in x


def test_plan_query_follows_the_compute_units_it_is_given(pkg):
    """compute_units replaces the device's count for the one call; 0 is the count the library holds (256 before any
    context exists, which is the case in a process without a device)."""
    n, replicas, noise = bp.case_shape("q32", "long")
    a = pkg.fused_plan_query(n, replicas, noise, compute_units=256)
    b = pkg.fused_plan_query(n, replicas, noise, compute_units=64)
    assert a["compute_units"] == 256 and b["compute_units"] == 64
    assert b["rounds"] == -(-b["workgroups"] // 64) and b != a
    assert pkg.fused_plan_query(n, replicas, noise, compute_units=256) == a            # nothing stuck from the call with 64
    held = pkg.fused_plan_query(n, replicas, noise)
    assert held == pkg.fused_plan_query(n, replicas, noise, compute_units=held["compute_units"])
    # a batch's noise tile is the 256-thread one, a lone lattice's the 512-thread one
    assert pkg.fused_plan_query((40, 11, 8), 2, True, 256)["tile_x"] == 32
    assert pkg.fused_plan_query((40, 11, 8), 1, True, 256)["tile_x"] == 64


@pytest.mark.parametrize("n,replicas,cus,pattern", [
    (None, 1, 0, "null"), ((8, 0, 8), 1, 0, "size"), ((8, 8, 8), 0, 0, "nreplicas"), ((8, 8, 8), 70000, 0, "nreplicas"),
    ((16384, 16384, 8), 1, 0, "32-bit"), ((8, 8, 8), 1, -1, "compute_units"),
])
def test_plan_query_rejects_bad_arguments(pkg, n, replicas, cus, pattern):
    lib = pkg._lib.load()
    out = (ctypes.c_int * 16)()
    n3 = (ctypes.c_int * 3)(*n) if n is not None else None
    assert lib.bflbm_fused_plan_query(n3, replicas, 0, cus, out) != 0
    msg = lib.bflbm_last_error().decode()
    assert msg.startswith("bflbm_fused_plan_query") and pattern in msg, msg
