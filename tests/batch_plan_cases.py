"""The case table of tests/test_batch_plans.py (CPU) and tests/test_gpu_batch_plans.py (GPU): which lattices and batch
sizes put every tile family of the one-pass batch kernels under every regime of the chunk planner, and what the library's
own planner (bflbm_fused_plan_query) must report for each.  The table was chosen for a device of 256 compute units."""

CUS = 256

# family -> lattice (nx, ny), noise, and what the plan must say about the tiling: four tile columns per replica, ragged in
# x and in y.  last_row: sites in y of the last tile row; last_cols: active columns of the last tile in x.
FAMILIES = {
    "q8": dict(nxy=(7, 200), noise=False, tile=(8, 64), ntx=1, nty=4, last_row=8, last_cols=7),
    "q16": dict(nxy=(12, 100), noise=False, tile=(16, 32), ntx=1, nty=4, last_row=4, last_cols=12),
    "q32": dict(nxy=(20, 50), noise=False, tile=(32, 16), ntx=1, nty=4, last_row=2, last_cols=20),
    "q64": dict(nxy=(70, 9), noise=False, tile=(64, 8), ntx=2, nty=2, last_row=1, last_cols=6),
    "n32": dict(nxy=(40, 11), noise=True, tile=(32, 8), ntx=2, nty=2, last_row=3, last_cols=8),
}

# regime -> nz, replicas and the properties of the plan.  chunks: planes of every chunk; pad: workgroups of the launched
# grid beyond the work list (they must leave); split: an XCD part boundary falls inside some replica's work list.
REGIMES = {
    "long": dict(nz=8, B=43, chunks=[8], workgroups=172, rounds=1, pad=4),
    "ragged": dict(nz=11, B=33, chunks=[4, 4, 3], workgroups=396, rounds=2, pad=4, split=True),
    "tail": dict(nz=7, B=3, chunks=[3, 3, 1]),
    "full": dict(nz=14, B=64, chunks=[14], workgroups=256, rounds=1, pad=0),
}

# (family, regime): every family under the first three; "full" (256 workgroups exactly, no padding) for q32 and n32 only
# (q8 would be 1.3 M sites there)
CASES = [(f, r) for f in FAMILIES for r in ("long", "ragged", "tail")] + [("q32", "full"), ("n32", "full")]


def case_shape(family, regime):
    """-> n (nx, ny, nz), replicas, noise"""
    fam, reg = FAMILIES[family], REGIMES[regime]
    return fam["nxy"] + (reg["nz"],), reg["B"], fam["noise"]


def chunk_planes(plan, nz):
    """Planes of every chunk of a plan over nz planes."""
    lens = [plan["planes_per_chunk"]] * (plan["chunks"] - 1) + [plan["last_chunk_planes"]]
    assert sum(lens) == nz, f"the chunks {lens} do not cover {nz} planes"
    return lens


def xcd_boundary_inside_a_replica(plan):
    """True where one of the seven boundaries between the XCD parts of the work list is not a replica boundary."""
    per, wpr, total = plan["per_xcd"], plan["workgroups_per_replica"], plan["workgroups"]
    return any(x * per < total and (x * per) % wpr != 0 for x in range(1, 8))


def check_tiling(plan, n, tile, ntx, nty, last_row, last_cols, **_):
    """The plan tiles the lattice as the family says."""
    what = f"{n}: "
    assert (plan["tile_x"], plan["tile_y"]) == tile, what + f"tile {plan['tile_x']} x {plan['tile_y']}, expected {tile}"
    assert (plan["ntx"], plan["nty"]) == (ntx, nty), what + f"{plan['ntx']} x {plan['nty']} tiles, expected {ntx} x {nty}"
    assert n[0] - (ntx - 1) * tile[0] == last_cols and n[1] - (nty - 1) * tile[1] == last_row, what + "raggedness of the table"
    assert 0 < last_cols < tile[0] and 0 < last_row < tile[1], what + "the last tiles must be partial in x and y"


def check_regime(plan, n, replicas, chunks, workgroups=None, rounds=None, pad=None, split=None, **_):
    """The plan has the regime's properties."""
    what = f"{n} x {replicas}: "
    assert chunk_planes(plan, n[2]) == chunks, what + f"chunks {chunk_planes(plan, n[2])}, expected {chunks}"
    assert plan["workgroups"] == replicas * plan["workgroups_per_replica"] == replicas * plan["ntx"] * plan["nty"] * len(chunks)
    assert plan["per_xcd"] == -(-plan["workgroups"] // 8) and plan["grid"] == 8 * plan["per_xcd"]
    assert plan["rounds"] == -(-plan["workgroups"] // plan["compute_units"])
    if workgroups is not None:
        assert plan["workgroups"] == workgroups, what + f"{plan['workgroups']} workgroups, expected {workgroups}"
    if rounds is not None:
        assert plan["rounds"] == rounds, what + f"{plan['rounds']} rounds, expected {rounds}"
    if pad is not None:
        assert plan["grid"] - plan["workgroups"] == pad, what + f"list padded by {plan['grid'] - plan['workgroups']}, expected {pad}"
    if split:
        assert xcd_boundary_inside_a_replica(plan), what + "every XCD part boundary is a replica boundary"


def check_case(plan, family, regime):
    n, replicas, _ = case_shape(family, regime)
    check_tiling(plan, n, **FAMILIES[family])
    check_regime(plan, n, replicas, **REGIMES[regime])


# Column order with a narrower last strip (fused_col): ntx = 5, 6, 7 at strips of 4 tiles -> a last strip of 1, 2, 3 tiles
STRIP_SHAPES = [((260, 9, 4), 5), ((330, 9, 4), 6), ((400, 9, 3), 7)]


def check_strips(plan, n, ntx):
    assert (plan["tile_x"], plan["tile_y"]) == (64, 8), f"{n}: tile {plan['tile_x']} x {plan['tile_y']}"
    assert plan["ntx"] == ntx and plan["sx"] == 4, f"{n}: ntx {plan['ntx']}, strips of {plan['sx']}; expected {ntx}, 4"
    assert plan["ntx"] - plan["sx"] == ntx - 4 and 1 <= ntx - 4 <= 3, f"{n}: last strip not 1..3 tiles wide"
    assert plan["nty"] == 2, f"{n}: {plan['nty']} tile rows"        # the strip order differs from row-major only with nty > 1
