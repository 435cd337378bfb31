"""Recorders of a ring, CPU side: the C-ABI surface (declared, exported, bound), the null-pointer refusals (which must
fail before any device is touched), the slab tables of a ring's spectrum trace through a stand-alone host program built
with the address and undefined-behaviour sanitizers, and the two new kernels in the gfx950 assembly (hipcc cross-compiles,
no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from device_listing import device_asm, kernel_of, mangled   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

RING_SYMBOLS = ["bflbm_ring_trace_create", "bflbm_ring_spectrum_create"]


def test_ring_recorder_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in RING_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    # declared with their groups, after the calls they stand beside
    assert header.index("Ensemble traces") < header.index("bflbm_batch_trace_create(") < header.index("bflbm_ring_trace_create(") < header.index("Interface traces")
    assert header.index("Spectrum traces") < header.index("bflbm_batch_spectrum_create(") < header.index("bflbm_ring_spectrum_create(")
    assert pkg._lib.SIGNATURES["bflbm_ring_trace_create"] == pkg._lib.SIGNATURES["bflbm_batch_trace_create"]
    assert pkg._lib.SIGNATURES["bflbm_ring_spectrum_create"] == pkg._lib.SIGNATURES["bflbm_batch_spectrum_create"]
    assert callable(pkg.RingLBM.trace) and callable(pkg.RingLBM.spectrum_trace)
    assert not hasattr(pkg.RingLBM, "interface_trace")        # columns cross slabs: out of scope


def test_ring_recorder_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    ring = ctypes.c_void_p(8)                                # never dereferenced: the other null argument is refused first
    va, vb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    calls = {
        "bflbm_ring_trace_create": [lambda: lib.bflbm_ring_trace_create(None, 1, 4, 0.0, ctypes.byref(h)),
                                    lambda: lib.bflbm_ring_trace_create(ring, 1, 4, 0.0, None)],
        "bflbm_ring_spectrum_create": [lambda: lib.bflbm_ring_spectrum_create(None, 1, va, vb, None, 0, 0, 1, 1, 4, ctypes.byref(h)),
                                       lambda: lib.bflbm_ring_spectrum_create(ring, 1, None, vb, None, 0, 0, 1, 1, 4, ctypes.byref(h)),
                                       lambda: lib.bflbm_ring_spectrum_create(ring, 1, va, None, None, 0, 0, 1, 1, 4, ctypes.byref(h)),
                                       lambda: lib.bflbm_ring_spectrum_create(ring, 1, va, vb, None, 0, 0, 1, 1, 4, None)],
    }
    for name, variants in calls.items():
        for call in variants:
            assert call() != 0, name
            msg = lib.bflbm_last_error().decode()
            assert "null" in msg and name in msg, (name, msg)
            assert not h.value


def test_structure_factor_null_pointers_are_refused(pkg):
    """The twelve bflbm_sf_* / bflbm_ring_sf_* calls: every null-argument refusal names its call and comes before any
    device is touched; the two _destroy calls take a null handle like free() and return 0."""
    lib = pkg._lib.load()
    h, n = ctypes.c_void_p(), ctypes.c_longlong()
    owner = ctypes.c_void_p(8)                               # never dereferenced: the other null argument is refused first
    va, vb = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(1)
    buf = (ctypes.c_double * 1)()
    for pre in ("bflbm_sf_", "bflbm_ring_sf_"):
        f = lambda name: getattr(lib, pre + name)
        calls = {
            "create": [lambda: f("create")(None, 1, va, vb, None, ctypes.byref(h)),
                       lambda: f("create")(owner, 1, None, vb, None, ctypes.byref(h)),
                       lambda: f("create")(owner, 1, va, None, None, ctypes.byref(h)),
                       lambda: f("create")(owner, 1, va, vb, None, None)],
            "reset": [lambda: f("reset")(None)],
            "accumulate": [lambda: f("accumulate")(None, 0, 0)],
            "nsamples": [lambda: f("nsamples")(None, ctypes.byref(n)), lambda: f("nsamples")(owner, None)],
            "get": [lambda: f("get")(None, 0, 1, buf), lambda: f("get")(owner, 0, 1, None)],
        }
        for name, variants in calls.items():
            for call in variants:
                assert call() != 0, pre + name
                msg = lib.bflbm_last_error().decode()
                assert "null argument" in msg and pre + name in msg, (pre + name, msg)
                assert not h.value
        assert f("destroy")(None) == 0


# ---- the slab tables -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path_factory.mktemp("tables") / "ring_spectrum_tables_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", str(out), os.path.join(ROOT, "tests", "ring_spectrum_tables_main.cpp")], check=True, timeout=600)
    return str(out)


@pytest.mark.parametrize("n,nslabs", [((9, 7, 12), 3), ((16, 128, 65), 2), ((8, 8, 8), 8)])
def test_slab_tables_partition_the_half_spectrum(tables_program, n, nslabs):
    """Every kind and zero_avg: the slabs' lists partition the half spectrum (minus k = 0 with zero_avg), no chunk crosses
    a bin, and the weighted counts summed over the slabs are the lone build's."""
    out = subprocess.run([tables_program] + [str(v) for v in n] + [str(nslabs)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "OK 8", (out.stdout[-1000:], out.stderr[-3000:])


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k_spectrum_collect", "k_spectrum_combine"])
def test_ring_spectrum_kernel_compiled_once_without_scratch(device_asm, kernel):
    body, meta = kernel_of(device_asm, mangled(kernel))
    assert not [l for l in body if "atomic" in l], f"{kernel} uses atomics"
    assert re.search(r"; ScratchSize: 0\b", meta), f"{kernel} spills to scratch"
    assert re.search(r"; LDSByteSize: 0\b", meta), f"{kernel} uses LDS"
    if kernel == "k_spectrum_collect":                       # 16 bytes per element, both ways
        assert [l for l in body if "global_load_dwordx4" in l] and [l for l in body if "global_store_dwordx4" in l]
