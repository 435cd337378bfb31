"""Where the steady-state loop of the full-tile unit-rate hand-over kernel k_fused_ho_unit<4,false> issues its memory
operations (no GPU needed: hipcc cross-compiles gfx950).  The arrangement was found by measurement (NOTES.md section 3.1g,
profiles/request_placement_ab.txt) and none of it shows in the source as such, so it is pinned on the assembly:

  * fifteen of the 19 outputs of fluid g are stored one march position late, as one run directly in front of the barrier,
    behind the density sums (+3.4 % at 512^3; behind the barrier or spread over the hold swap the same stores lost or gained
    nothing);
  * the last four are stored at once, behind the requests of the g half, so that the waits at the loop head cover loads only;
  * the g half is still requested as one burst (every spread of it lost 1-3 %).
"""
import re

from device_listing import device_asm, kernel_of, steady_loop   # noqa: F401  (device_asm: the listing fixture)

SYMBOL = r"_Z15k_fused_ho_unitILi4ELb0EE"
DEFERRED, AT_ONCE = 15, 4


def _loop(device_asm):
    body, _ = kernel_of(device_asm, r"^%s\w*:" % SYMBOL)
    lo, hi = steady_loop(body)
    ops = []
    for l in body[lo:hi]:
        t = l.split()[0] if l.split() else ""
        if t.startswith("global_load"):
            ops.append(("L", l))
        elif t.startswith("global_store"):
            ops.append(("S", l))
        elif t.startswith("s_barrier"):
            ops.append(("B", l))
        elif t.startswith("s_waitcnt") and "vmcnt" in l:
            ops.append(("W", int(re.search(r"vmcnt\((\d+)\)", l).group(1))))
        elif t.startswith(("v_", "ds_")):
            ops.append(("x", l))
    return ops


def _memory(ops):
    return [o for o in ops if o[0] != "x"]


def _deferred_run(ops):
    """(first, last + 1) of the run of stores that ends at the loop's barrier."""
    bars = [i for i, (k, _) in enumerate(ops) if k == "B"]
    assert len(bars) == 1, "the steady-state loop has one barrier"
    first = bars[0]
    while first > 0 and ops[first - 1][0] == "S":
        first -= 1
    return first, bars[0]


def test_longest_run_of_requests_is_the_burst_of_the_g_half(device_asm):
    ops = _loop(device_asm)
    runs = [len(m.group(0)) for m in re.finditer(r"L+", "".join(k for k, _ in ops))]
    print("runs of consecutive global loads in the steady-state loop:", runs)
    # the g half stays a burst of at most 19 (18 + 1 in the shipped listing): no block of requests grew beyond it ...
    assert max(runs) <= 19, runs
    # ... and it is still there: requests of the g half placed between the stages of its relaxation lost 1.0-2.8 % at 512^3
    assert max(runs) >= 15, runs


def test_deferred_g_stores_stand_in_front_of_the_barrier(device_asm):
    ops = _memory(_loop(device_asm))
    first, bar = _deferred_run(ops)
    # the arrangement that gained: all deferred outputs as one run of non-temporal stores between the density sums and the barrier
    assert bar - first == DEFERRED, f"{bar - first} stores in front of the barrier"
    assert all(re.search(r"\bnt\b", l) for _, l in ops[first:bar])
    # no request of the next plane stands between the loop head and the run: the stores meet an empty queue
    assert sum(1 for k, _ in ops[:first] if k == "S") == 0, "stores in front of the deferred run"


def test_waits_cover_loads_only(device_asm):
    ops = _memory(_loop(device_asm))
    first, bar = _deferred_run(ops)
    head_end = min(i for i, (k, _) in enumerate(ops) if k in "LS")
    head = [v for k, v in ops[:head_end] if k == "W"]
    print("vmcnt waits at the loop head:", head)
    # the four outputs stored at once are younger than the last request of the g half: the head never drains them
    assert head and min(head) >= AT_ONCE, f"the loop head waits for stores: {head}"
    tail = ops[max(i for i, (k, _) in enumerate(ops) if k == "L") + 1:]
    assert sum(1 for k, _ in tail if k == "S") >= AT_ONCE, "the stores behind the last request of the g half are gone"
    # every wait between the first deferred store and the first request of the f half leaves the deferred stores issued so far in flight
    nxt = min(i for i, (k, _) in enumerate(ops) if k == "L" and i > bar)
    issued = 0
    for k, v in ops[first:nxt]:
        if k == "S":
            issued += 1
        elif k == "W":
            assert v >= min(issued, DEFERRED), f"vmcnt({v}) behind {issued} deferred stores"
