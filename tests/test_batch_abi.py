"""Replica batches, CPU side: the C-ABI surface, the argument checks of bflbm_batch_create (which must fail before any
device is touched) and the compiled batch kernels (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re

import pytest

from device_listing import device_asm, kernel_of   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCH_SYMBOLS = ["bflbm_batch_create", "bflbm_batch_destroy", "bflbm_batch_size", "bflbm_batch_replica",
                 "bflbm_batch_set_schedule", "bflbm_batch_resolved_schedule", "bflbm_batch_step", "bflbm_batch_sync",
                 "bflbm_fused_plan_query", "bflbm_sweep_plan_query"]


def test_batch_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in BATCH_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert hasattr(pkg, "BatchLBM") and "BatchLBM" in pkg.__all__


def _create(pkg, params, nrep, n):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n3 = (ctypes.c_int * 3)(*n) if n is not None else None
    rc = lib.bflbm_batch_create(params, nrep, n3, 0, ctypes.byref(h))
    return rc, lib.bflbm_last_error().decode(), h


@pytest.mark.parametrize("case,nrep,n,pattern", [
    ("null params", 2, (8, 8, 8), "null"),
    ("no replicas", 0, (8, 8, 8), "nreplicas"),
    ("negative replicas", -3, (8, 8, 8), "nreplicas"),
    ("null size", 2, None, "null"),
    ("zero size", 2, (8, 0, 8), "size"),
    ("negative size", 2, (-1, 8, 8), "size"),
    ("32-bit offsets", 2, (16384, 16384, 8), "32-bit"),
])
def test_batch_create_rejects_before_touching_a_device(pkg, case, nrep, n, pattern):
    arr = None if case == "null params" else (pkg.Params * 2)(pkg.default_params(), pkg.default_params())
    rc, msg, h = _create(pkg, arr, nrep, n)
    assert rc != 0 and not h.value, case
    assert msg.startswith("bflbm_batch_create") and pattern in msg, msg


def test_batch_python_arguments(pkg):
    with pytest.raises(ValueError):
        pkg.BatchLBM(8, params={"alpha0": 1.0})                        # one dict needs replicas=
    with pytest.raises(ValueError):
        pkg.BatchLBM(8, params=[{}, {}], replicas=3)


BATCH_KERNELS = [
    r"_Z15k_density_batchPK8BatchRec",
    r"_Z15k_collide_batchILb0EE",
    r"_Z15k_collide_batchILb1EE",
    r"_Z13k_fused_batchILi64ELi8ELi0EE",
    r"_Z13k_fused_batchILi32ELi16ELi0EE",
    r"_Z13k_fused_batchILi16ELi32ELi0EE",
    r"_Z13k_fused_batchILi8ELi64ELi0EE",
    r"_Z13k_fused_batchILi32ELi8ELi1EE",
]


@pytest.mark.parametrize("symbol", BATCH_KERNELS)
def test_batch_kernel_compiled_without_scratch(device_asm, symbol):
    body, meta = kernel_of(device_asm, r"^%s\w*:" % symbol, "batch kernel")
    assert re.search(r"; ScratchSize: 0\b", meta), f"{symbol} spills to scratch"
    body = "\n".join(body)
    assert "s_load_dword" in body                                        # the per-replica record: scalar loads
