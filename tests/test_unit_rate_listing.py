"""The compiled unit-rate kernels (no GPU needed: hipcc cross-compiles gfx950): the quiet one-pass kernels and the batch's
pass B have a unit-rate form, none of them uses scratch or spills more registers than the generic kernel it stands in for
(the lone two-pass k_collide would: it has none, csrc/bflbm_kernels.h), and in the hand-over kernel the folding happened (fewer vector instructions in the
steady-state loop than the generic kernel) while the spread requests of the f half are still placed."""
import re

import pytest

from device_listing import device_asm, kernel_of, spills, steady_loop   # noqa: F401  (device_asm: the listing fixture)

# unit-rate kernel -> the generic kernel it stands in for
UNIT_KERNELS = {
    r"_Z20k_collide_batch_unitPK8BatchRec": r"_Z15k_collide_batchILb0EE",
    r"_Z12k_fused_unitILi64ELi8EE": r"_Z7k_fusedILi64ELi8ELi0EE",
    r"_Z12k_fused_unitILi32ELi16EE": r"_Z7k_fusedILi32ELi16ELi0EE",
    r"_Z12k_fused_unitILi16ELi32EE": r"_Z7k_fusedILi16ELi32ELi0EE",
    r"_Z12k_fused_unitILi8ELi64EE": r"_Z7k_fusedILi8ELi64ELi0EE",
    r"_Z18k_fused_batch_unitILi64ELi8EE": r"_Z13k_fused_batchILi64ELi8ELi0EE",
    r"_Z18k_fused_batch_unitILi32ELi16EE": r"_Z13k_fused_batchILi32ELi16ELi0EE",
    r"_Z18k_fused_batch_unitILi16ELi32EE": r"_Z13k_fused_batchILi16ELi32ELi0EE",
    r"_Z18k_fused_batch_unitILi8ELi64EE": r"_Z13k_fused_batchILi8ELi64ELi0EE",
    r"_Z15k_fused_ho_unitILi4ELb0EE": r"_Z10k_fused_hoILi4ELi0ELb0EE",
    r"_Z15k_fused_ho_unitILi4ELb1EE": r"_Z10k_fused_hoILi4ELi0ELb1EE",
}


def _kernel(lines, symbol):
    return kernel_of(lines, r"^%s\w*:" % symbol)


@pytest.mark.parametrize("symbol", list(UNIT_KERNELS))
def test_unit_rate_kernel_compiled_without_scratch_or_more_spills(device_asm, symbol):
    _, meta = _kernel(device_asm, symbol)
    assert re.search(r"; ScratchSize: 0\b", meta), f"{symbol} spills to scratch"
    unit, gen = spills(device_asm, symbol), spills(device_asm, UNIT_KERNELS[symbol])
    print(symbol, "sgpr spills, vgpr spills, scratch bytes:", unit, "generic:", gen)
    assert unit[2] == 0
    assert unit[0] <= gen[0] and unit[1] <= gen[1], (unit, gen)


def _valu(body, lo, hi):
    return sum(1 for l in body[lo:hi] if l.split() and l.split()[0].startswith("v_"))


@pytest.mark.parametrize("rag", [0, 1])
def test_handover_unit_kernel_lost_the_ghost_mode_arithmetic_and_kept_the_spread(device_asm, rag):
    gen, _ = _kernel(device_asm, r"_Z10k_fused_hoILi4ELi0ELb%dEE" % rag)
    unit, _ = _kernel(device_asm, r"_Z15k_fused_ho_unitILi4ELb%dEE" % rag)
    (glo, ghi), (ulo, uhi) = steady_loop(gen), steady_loop(unit)
    vg, vu = _valu(gen, glo, ghi), _valu(unit, ulo, uhi)
    print(f"rag={rag}: VALU instructions in the steady-state loop {vg} -> {vu}")
    # nine ghost rows of d_moments (about 8 additions each), their relaxation (3 each) and what d_population_terms does with
    # them, for two fluids: well over 150 instructions; the two loops hold the same loads and stores
    assert vg - vu >= 150, (vg, vu)
    for op in ("global_load", "global_store", "ds_"):
        assert sum(op in l for l in gen[glo:ghi]) == sum(op in l for l in unit[ulo:uhi]), op
    if rag:
        return
    spaced, gap, pending = 0, 0, False
    for l in unit[ulo:uhi]:
        t = l.split()[0] if l.split() else ""
        if t.startswith("global_load") or t.startswith("global_store"):
            if pending and gap >= 20:
                spaced += 1
            pending, gap = t.startswith("global_load"), 0
        elif t.startswith("v_"):
            gap += 1
    assert spaced >= 15, f"only {spaced} loads of the steady-state loop stand alone between arithmetic"
