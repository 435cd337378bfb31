"""The case table of tests/test_sweep_plans.py (CPU) and tests/test_gpu_sweep_plans.py (GPU): lone lattices and one ring of
slabs that put the plane-marching sweeps -- the hand-over kernel (64 x 4 tiles, chunks of at least 4 planes) and the one-pass
exact kernel (64 x 8 tiles, strips of 4) -- under the plans of large lattices, and what the library's own planner
(bflbm_sweep_plan_query) must report for each.  The table was chosen for a device of 256 compute units; the planner
confirmed every shape as first chosen, none had to be replaced."""

CUS = 256

# regime -> shape and the properties of the hand-over plan.  chunks: planes of every chunk; pad: workgroups of the launched
# grid beyond the work list (they must leave); last_cols / last_row: active columns / rows of the last tile in x / y.
#   long:   ONE chunk of 40 planes (42 march positions: the four-slot density ring wraps ten times, 38 planes read frames),
#           exactly 256 workgroups, one round, no padding -- the plan of 256^3
#   rounds: ntx = 8 as at 512^3, one chunk of 24, 512 workgroups = 2 rounds (fused_map sees a second round)
#   cut:    an odd tile count in x, chunks of 9, 9, 8 planes, 885 workgroups = 4 rounds (the last one partial), padded by 3
#   cut7:   ntx = 7, three chunks of 11, 777 workgroups = 4 rounds, padded by 7
HANDOVER = {
    "long": dict(n=(256, 256, 40), ntx=4, nty=64, chunks=[40], workgroups=256, rounds=1, pad=0, last_cols=64, last_row=4),
    "long_ragged": dict(n=(250, 254, 40), ntx=4, nty=64, chunks=[40], workgroups=256, rounds=1, pad=0, last_cols=58, last_row=2),
    "rounds": dict(n=(512, 256, 24), ntx=8, nty=64, chunks=[24], workgroups=512, rounds=2, pad=0, last_cols=64, last_row=4),
    "rounds_ragged": dict(n=(500, 254, 24), ntx=8, nty=64, chunks=[24], workgroups=512, rounds=2, pad=0, last_cols=52, last_row=2),
    "cut": dict(n=(320, 236, 26), ntx=5, nty=59, chunks=[9, 9, 8], workgroups=885, rounds=4, pad=3, last_cols=64, last_row=4),
    "cut7": dict(n=(448, 148, 33), ntx=7, nty=37, chunks=[11, 11, 11], workgroups=777, rounds=4, pad=7, last_cols=64, last_row=4),
}

# The ring: 2 slabs of 12 planes.  Each slab's interior sweep is ONE chunk of 8 planes over 768 tile columns = 3 rounds (the
# min_slab_rounds branch of plan_chunks, which no small slab reaches with a chunk longer than 5); its boundary pairs are one
# launch of two 2-plane chunks whose starts are 10 planes apart.
NSLABS, SLAB_PLANES = 2, 12
RING = {
    "ring": dict(n=(512, 384, 24), ntx=8, nty=96, chunks=[8], workgroups=768, rounds=3, pad=0, last_cols=64, last_row=4,
                 pair_planes=2, pair_stride=10),
    "ring_ragged": dict(n=(500, 382, 24), ntx=8, nty=96, chunks=[8], workgroups=768, rounds=3, pad=0, last_cols=52, last_row=2,
                        pair_planes=2, pair_stride=10),
}

# The one-pass exact kernel on the lone shapes: tiles 64 x 8; sx: strip width of the column order (sx < ntx: strips)
FUSED = {
    "long": dict(n=(256, 256, 40), ntx=4, nty=32, sx=4, chunks=[20, 20], workgroups=256, rounds=1, pad=0),
    "rounds": dict(n=(512, 256, 24), ntx=8, nty=32, sx=4, chunks=[24], workgroups=256, rounds=1, pad=0),
    "cut": dict(n=(320, 236, 26), ntx=5, nty=30, sx=4, chunks=[9, 9, 8], workgroups=450, rounds=2, pad=6, last_strip=1),
}
# ... and on a slab of the ring: 768 workgroups in 3 rounds, two chunks of 4, the same boundary-pair launch
FUSED_RING = dict(n=(512, 384, 24), ntx=8, nty=48, sx=4, chunks=[4, 4], workgroups=768, rounds=3, pad=0, pair_planes=2, pair_stride=10)


def chunk_planes(plan):
    """Planes of every chunk of the interior sweep of a plan; the chunks must tile their range without gaps."""
    assert plan["chunk_stride"] == plan["planes_per_chunk"], f"chunks of {plan['planes_per_chunk']} planes {plan['chunk_stride']} apart"
    return [plan["planes_per_chunk"]] * (plan["chunks"] - 1) + [plan["last_chunk_planes"]]


def chunk_ranges(plan, first=0):
    """[(first plane, one past the last)] of every chunk of the interior sweep, the sweep starting at plane `first`."""
    out, z = [], first
    for planes in chunk_planes(plan):
        out.append((z, z + planes))
        z += planes
    return out


def check_plan(plan, case, tile, interior_planes=None):
    """The plan has the tiling and the regime the table says."""
    n = case["n"]
    what = f"{n}: "
    planes = n[2] if interior_planes is None else interior_planes
    assert (plan["tile_x"], plan["tile_y"]) == tile, what + f"tile {plan['tile_x']} x {plan['tile_y']}, expected {tile}"
    assert (plan["ntx"], plan["nty"]) == (case["ntx"], case["nty"]), what + f"{plan['ntx']} x {plan['nty']} tiles, expected {case['ntx']} x {case['nty']}"
    assert plan["ntx"] == -(-n[0] // tile[0]) and plan["nty"] == -(-n[1] // tile[1]), what + "tile counts against the lattice"
    lens = chunk_planes(plan)
    assert lens == case["chunks"] and sum(lens) == planes, what + f"chunks {lens}, expected {case['chunks']} over {planes} planes"
    assert plan["workgroups"] == plan["ntx"] * plan["nty"] * len(lens) == case["workgroups"], what + f"{plan['workgroups']} workgroups, expected {case['workgroups']}"
    assert plan["rounds"] == -(-plan["workgroups"] // plan["compute_units"]) == case["rounds"], what + f"{plan['rounds']} rounds, expected {case['rounds']}"
    assert plan["per_xcd"] == -(-plan["workgroups"] // 8) and plan["grid"] == 8 * plan["per_xcd"], what + "work list"
    assert plan["grid"] - plan["workgroups"] == case["pad"], what + f"list padded by {plan['grid'] - plan['workgroups']}, expected {case['pad']}"
    if "sx" in case:
        assert plan["sx"] == case["sx"], what + f"strips of {plan['sx']}, expected {case['sx']}"
        if "last_strip" in case:
            assert plan["ntx"] % plan["sx"] == case["last_strip"], what + "width of the last strip"
    else:
        assert plan["sx"] == plan["ntx"], what + "the hand-over kernel orders its columns row-major"
    if "last_cols" in case:
        assert n[0] - (case["ntx"] - 1) * tile[0] == case["last_cols"] and n[1] - (case["nty"] - 1) * tile[1] == case["last_row"], \
            what + "raggedness of the table"
    assert (plan["pair_planes"], plan["pair_stride"]) == (case.get("pair_planes", 0), case.get("pair_stride", 0)), \
        what + f"boundary pairs {plan['pair_planes']} planes, {plan['pair_stride']} apart"


def check_handover(plan, regime):
    check_plan(plan, HANDOVER[regime], (64, 4))


def check_ring(plan, regime):
    check_plan(plan, RING[regime], (64, 4), interior_planes=SLAB_PLANES - 4)


def check_fused(plan, regime):
    check_plan(plan, FUSED[regime], (64, 8))


def check_fused_ring(plan):
    check_plan(plan, FUSED_RING, (64, 8), interior_planes=SLAB_PLANES - 4)
