"""The compiled reduction kernels of the slab observables (csrc/bflbm_reduce.h and its users; no GPU needed: hipcc
cross-compiles gfx950).  Conditions, not measurements: the workgroup tree holds NV columns of 256 doubles in LDS and
nothing else, and a kernel of this layer that spilled would pay for it on every sample of every recorder.

The three trace kernels have their scratch check in test_trace_abi.py; their LDS is checked here."""
import pytest

from device_listing import device_asm, kernel_of, lds_bytes, mangled, scratch_size   # noqa: F401  (device_asm: the listing fixture)

SUM, MINMAX, ABSMAX = "NS_7SumRuleE", "NS_10MinMaxRuleE", "NS_10AbsMaxRuleE"

# (kernel, what follows its name in the label, NV); LDS = 8 * 256 * NV: the tree's columns
STAGE1 = [("k_moments", "E", 20), ("k_tanhfit", "E", 15), ("k_flowfit", "E", 2), ("k_minmax", "E", 2), ("k_reduce", "P", 5),
          ("k_total_absmax", "P", 1), ("k_trace_moments", "E", 12), ("k_trace_moments_batch", "E", 12)]
STAGE2 = [("k_plane_partials", "ILi20E%sE" % SUM, 20), ("k_plane_partials", "ILi15E%sE" % SUM, 15),
          ("k_plane_partials", "ILi2E%sE" % SUM, 2), ("k_plane_partials", "ILi2E%sE" % MINMAX, 2),
          ("k_trace_finish", "E", 12)]


@pytest.mark.parametrize("kernel,tail,nv", STAGE1 + STAGE2, ids=lambda v: str(v))
def test_reduction_kernel_has_one_definition_no_scratch_and_the_lds_of_its_tree(device_asm, kernel, tail, nv):
    _, meta = kernel_of(device_asm, mangled(kernel, tail), "reduction kernel")
    assert scratch_size(meta) == 0, f"{kernel}{tail} spills to scratch"
    # the sum kernels 8 * 256 * NV; the (min, max) pair 4096 (NV = 2) and the absmax 2048 (NV = 1) by the same formula
    assert lds_bytes(meta) == 8 * 256 * nv, f"{kernel}{tail}: LDS is not the tree's {nv} columns of 256 doubles"
