"""The compiled schedule of the hand-over kernel (no GPU needed: hipcc cross-compiles gfx950).

With one wave per SIMD nothing hides a conservative wait, and two faults of exactly that kind were found in the
generated code of this kernel (NOTES.md section 3.1b, "Two faults in the generated schedule"): a `vmcnt(0)` at the
head of the march loop that drained the stores of every position, and a pulled ring scheduled as 38 load-wait-add
triples.  Neither shows in the source, so the properties are pinned on the assembly here."""
import re

import pytest

from device_listing import device_asm, kernel_of, steady_loop   # noqa: F401  (device_asm: the listing fixture)



def _kernel(lines, mode):
    return kernel_of(lines, r"^_Z10k_fused_hoILi4ELi%dELb0EE.*:" % mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_handover_kernel_schedule(device_asm, mode):
    body, meta = _kernel(device_asm, mode)
    assert re.search(r"; ScratchSize: 0\b", meta), "the hand-over kernel spills to scratch"
    lo, hi = steady_loop(body)
    waits = [(i, int(re.search(r"vmcnt\((\d+)\)", body[i]).group(1))) for i in range(lo, hi) if "s_waitcnt" in body[i] and "vmcnt" in body[i]]
    first_store = min(i for i in range(lo, hi) if "global_store" in body[i])
    first_load = min(i for i in range(lo, hi) if "global_load" in body[i])
    head = [w for i, w in waits if i < min(first_store, first_load)]
    # the head waits for the loads of the previous position only: the 19 stores of fluid g stay in flight
    assert head and min(head) >= 19, f"loop head drains the stores again: {head}"
    # the pulled ring of the chunk-boundary planes is one batch: its waits count down once, so vmcnt(0) appears once
    assert sum(1 for _, w in waits if w == 0) <= 1, [w for _, w in waits]


def test_quiet_kernel_requests_the_f_half_between_the_arithmetic(device_asm):
    """Round 3 (NOTES.md section 3.1f): a lone wave that issues 19 requests back to back stands at the issue for as long as
    the request queue takes to make room; the quiet kernel therefore requests the f half of the next plane one load every
    30 VALU instructions of the relaxation (sched_group_barrier).  Left to itself the compiler hoists the loads into one
    burst again, so the spacing is pinned here: at least 15 loads of the steady-state loop are followed by 20 or more VALU
    instructions before the next vector-memory instruction."""
    body, _ = _kernel(device_asm, 0)
    lo, hi = steady_loop(body)
    spaced, gap, pending = 0, 0, False
    for l in body[lo:hi]:
        t = l.split()[0] if l.split() else ""
        if t.startswith("global_load") or t.startswith("global_store"):
            if pending and gap >= 20:
                spaced += 1
            pending, gap = t.startswith("global_load"), 0
        elif t.startswith("v_"):
            gap += 1
    assert spaced >= 15, f"only {spaced} loads of the steady-state loop stand alone between arithmetic"
