"""Ensemble traces, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must fail
before any device is touched), analysis.msd, and the compiled trace kernels (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from device_listing import device_asm, kernel_of, mangled   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACE_SYMBOLS = ["bflbm_trace_create", "bflbm_batch_trace_create", "bflbm_trace_destroy", "bflbm_trace_sample",
                 "bflbm_trace_reset", "bflbm_trace_count", "bflbm_trace_read"]


def test_trace_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in TRACE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert re.search(r"#define\s+BFLBM_TRACE_NREC\s+12\b", header) and pkg._lib.TRACE_NREC == 12
    assert hasattr(pkg, "Trace") and "Trace" in pkg.__all__


def test_trace_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    rec = (ctypes.c_double * 12)()
    calls = {
        "bflbm_trace_create": lambda: lib.bflbm_trace_create(None, 1, 4, 0.0, ctypes.byref(h)),
        "bflbm_trace_create (out)": lambda: lib.bflbm_trace_create(None, 1, 4, 0.0, None),
        "bflbm_batch_trace_create": lambda: lib.bflbm_batch_trace_create(None, 1, 4, 0.0, ctypes.byref(h)),
        "bflbm_trace_sample": lambda: lib.bflbm_trace_sample(None),
        "bflbm_trace_reset": lambda: lib.bflbm_trace_reset(None),
        "bflbm_trace_count": lambda: lib.bflbm_trace_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_trace_read": lambda: lib.bflbm_trace_read(None, 0, 1, rec, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name.split(" ")[0] in msg, (name, msg)
        assert not h.value
    assert lib.bflbm_trace_destroy(None) == 0            # like every destroy of the ABI: nothing to do


def test_msd_against_a_double_loop(pkg):
    rng = np.random.default_rng(11)
    r = rng.standard_normal((2, 40, 3)).cumsum(axis=1)
    max_lag = 17
    got = pkg.analysis.msd(r, max_lag)
    assert got.shape == (2, max_lag + 1)
    want = np.zeros((2, max_lag + 1))
    for a in range(2):
        for k in range(1, max_lag + 1):
            acc = 0.0
            for t in range(40 - k):
                d = r[a, t + k] - r[a, t]
                acc += float(d @ d)
            want[a, k] = acc / (40 - k)
    assert np.all(got[:, 0] == 0.0)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(pkg.analysis.msd(r[0], 3), want[0, :4], rtol=1e-13)
    with pytest.raises(ValueError):
        pkg.analysis.msd(r, 40)


@pytest.mark.parametrize("kernel", ["k_trace_moments", "k_trace_moments_batch", "k_trace_finish"])
def test_trace_kernel_compiled_without_scratch(device_asm, kernel):
    _, meta = kernel_of(device_asm, mangled(kernel), "trace kernel")
    assert re.search(r"; ScratchSize: 0\b", meta), f"{kernel} spills to scratch"
