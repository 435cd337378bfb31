"""Ensemble structure factors, CPU side: the C-ABI surface (declared, exported, bound), the refusals that must fail before
any device is touched, and the compiled kernels (hipcc cross-compiles gfx950, no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from device_listing import device_asm, kernel_of, mangled, scratch_size   # noqa: F401  (device_asm: the listing fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

SYMBOLS = ["bflbm_batch_sf_create", "bflbm_batch_sf_destroy", "bflbm_batch_sf_reset", "bflbm_batch_sf_accumulate",
           "bflbm_batch_sf_nsamples", "bflbm_batch_sf_get", "bflbm_batch_get_hydrovs", "bflbm_batch_get_hydrovsbar"]


def test_batch_sf_symbols_exported_and_declared(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    assert re.search(r"typedef\s+struct\s+bflbm_batch_sf\s+bflbm_batch_sf\s*;", header)      # the ninth name of the group
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/bflbm.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert re.search(r"#define\s+BFLBM_ABI_VERSION\s+1\b", header) and lib.bflbm_abi_version() == 1
    assert hasattr(pkg.structfact, "BatchStructFact") and issubclass(pkg.structfact.BatchStructFact, pkg.structfact.StructFact)
    assert pkg.BatchStructFact is pkg.structfact.BatchStructFact and "BatchStructFact" in pkg.__all__
    assert callable(pkg.BatchLBM.structfact)


def test_library_does_not_link_hipfft():
    out = subprocess.run(["readelf", "-d", os.path.join(CSRC, "libbflbm.so")], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("readelf not available")
    assert "hipfft" not in out.stdout.lower()


def test_batch_sf_refusals_touch_no_device(pkg):
    """Null pointers and out-of-range arguments: refused with a message naming the call, the out-handle stays null.
    `fake` stands for a batch; a call that dereferenced it would not get as far as the message."""
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n = ctypes.c_longlong()
    buf = (ctypes.c_double * 8)()
    one = (ctypes.c_int * 1)(0)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    I = ctypes.c_int

    def create(b=fake, npairs=1, a=one, bb=one, lb=0, every=0, out=ctypes.byref(h)):
        return lib.bflbm_batch_sf_create(b, npairs, a, bb, None, lb, every, out)

    calls = {
        "bflbm_batch_sf_create null batch": (lambda: create(b=None), "null"),
        "bflbm_batch_sf_create null var_a": (lambda: create(a=None), "null"),
        "bflbm_batch_sf_create null var_b": (lambda: create(bb=None), "null"),
        "bflbm_batch_sf_create null out": (lambda: create(out=None), "null"),
        "bflbm_batch_sf_create npairs 0": (lambda: create(npairs=0), "1..32"),
        "bflbm_batch_sf_create npairs 33": (lambda: create(npairs=33, a=(I * 33)(), bb=(I * 33)()), "1..32"),
        "bflbm_batch_sf_create var 22": (lambda: create(a=(I * 1)(22)), "hydrovs"),
        "bflbm_batch_sf_create var -1": (lambda: create(bb=(I * 1)(-1)), "hydrovs"),
        "bflbm_batch_sf_create var 9 of hydrovsbar": (lambda: create(a=(I * 1)(9), lb=1), "hydrovsbar"),
        "bflbm_batch_sf_create every -1": (lambda: create(every=-1), "every"),
        "bflbm_batch_sf_reset": (lambda: lib.bflbm_batch_sf_reset(None), "null"),
        "bflbm_batch_sf_accumulate": (lambda: lib.bflbm_batch_sf_accumulate(None, 0), "null"),
        "bflbm_batch_sf_nsamples": (lambda: lib.bflbm_batch_sf_nsamples(None, ctypes.byref(n)), "null"),
        "bflbm_batch_sf_nsamples null n": (lambda: lib.bflbm_batch_sf_nsamples(fake, None), "null"),
        "bflbm_batch_sf_get": (lambda: lib.bflbm_batch_sf_get(None, -1, 0, 1, buf), "null"),
        "bflbm_batch_sf_get null dst": (lambda: lib.bflbm_batch_sf_get(fake, -1, 0, 1, None), "null"),
        "bflbm_batch_get_hydrovs": (lambda: lib.bflbm_batch_get_hydrovs(None, buf, 1), "null"),
        "bflbm_batch_get_hydrovs null dst": (lambda: lib.bflbm_batch_get_hydrovs(fake, None, 1), "null"),
        "bflbm_batch_get_hydrovs ncomp 0": (lambda: lib.bflbm_batch_get_hydrovs(fake, buf, 0), "ncomp"),
        "bflbm_batch_get_hydrovs ncomp 23": (lambda: lib.bflbm_batch_get_hydrovs(fake, buf, 23), "ncomp"),
        "bflbm_batch_get_hydrovsbar": (lambda: lib.bflbm_batch_get_hydrovsbar(None, buf, 1), "null"),
        "bflbm_batch_get_hydrovsbar ncomp 0": (lambda: lib.bflbm_batch_get_hydrovsbar(fake, buf, 0), "ncomp"),
        "bflbm_batch_get_hydrovsbar ncomp 10": (lambda: lib.bflbm_batch_get_hydrovsbar(fake, buf, 10), "ncomp"),
    }
    for name, (call, word) in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert word in msg and name.split(" ")[0] in msg, (name, msg)
        assert not h.value, name
    assert lib.bflbm_batch_sf_destroy(None) == 0         # like every destroy of the ABI: nothing to do


def _scratch_size(asm, kernel, template_arg=None):
    """ScratchSize of the one definition of `kernel` (Itanium mangling: <length><name>, then ILi<N>E for <N>)."""
    tail = r"ILi%dEE" % template_arg if template_arg is not None else r"E?"
    return scratch_size(kernel_of(asm, mangled(kernel, tail))[1])


@pytest.mark.parametrize("kernel,arg", [("k_sf_accumulate", None), ("k_sf_expand", None), ("k_observe_batch", 0)])
def test_batch_sf_kernel_compiled_without_scratch(device_asm, kernel, arg):
    assert _scratch_size(device_asm, kernel, arg) == 0, f"{kernel} spills to scratch"


def test_observe_batch_hydrovs_spills_no_more_than_k_observe(device_asm):
    assert _scratch_size(device_asm, "k_observe_batch", 2) <= _scratch_size(device_asm, "k_observe", 2)
