"""The gfx950 assembly listing of csrc/bflbm.hip for the CPU suite (no GPU needed: hipcc cross-compiles), compiled once per
test process however many modules import the fixture, and the parsers the listing checks share.

A module that checks compiled kernels does `from device_listing import device_asm  # noqa: F401` and takes `device_asm`
as an argument of its tests: the lines of the listing.  Nobody changes them."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def listing():
    """The lines of the device-only listing (about a minute and 15 MB; cached for the life of the process)."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bflbm.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w",
                        "--cuda-device-only", "-S", "-o", out, "bflbm.hip"], cwd=CSRC, check=True, timeout=600)
        with open(out) as f:
            return f.read().split("\n")


@pytest.fixture(scope="module")
def device_asm():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return listing()


def mangled(kernel, tail="E"):
    """The label of a kernel by name, in a namespace or not (Itanium mangling: <length><name>; `tail` is what follows the
    name: "E" or nothing for a plain kernel, "ILi<N>EE" for its instantiation with <N>)."""
    return r"^_Z\w*?%d%s%s\w*:" % (len(kernel), kernel, tail)


def kernels(lines, label):
    """Every definition whose label matches: [(match, trailer)].  The trailer is what the compiler prints after the kernel
    (register counts, ScratchSize, LDSByteSize), never its instructions."""
    label = re.compile(label)
    out = []
    for s in [i for i, l in enumerate(lines) if label.match(l)]:
        end = [i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end")][0]
        out.append((label.match(lines[s]), "\n".join(lines[end:end + 120])))
    return out


def kernel_of(lines, label, what="kernel"):
    """(body, trailer) of the ONE definition whose label matches."""
    label = re.compile(label)
    starts = [i for i, l in enumerate(lines) if label.match(l)]
    assert len(starts) == 1, f"{what} {label.pattern}: {len(starts)} definitions in the gfx950 assembly"
    end = [i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end")][0]
    return lines[starts[0]:end], "\n".join(lines[end:end + 120])


def _trailer_int(trailer, key):
    m = re.search(r"; %s: (\d+)\b" % key, trailer)
    assert m, f"no {key} line"
    return int(m.group(1))


def scratch_size(trailer):
    return _trailer_int(trailer, "ScratchSize")


def lds_bytes(trailer):
    return _trailer_int(trailer, "LDSByteSize")


def spills(lines, symbol):
    """(sgpr_spill_count, vgpr_spill_count, private_segment_fixed_size) of a kernel from the code object metadata."""
    at = [i for i, l in enumerate(lines) if re.match(r"\s+\.name:\s+%s\w*$" % symbol, l)]
    assert len(at) == 1, symbol
    lo = max(i for i in range(at[0]) if lines[i].startswith("  - .")) if any(lines[i].startswith("  - .") for i in range(at[0])) else 0
    hi = min([i for i in range(at[0] + 1, len(lines)) if lines[i].startswith("  - .") or lines[i].startswith("amdhsa.")] + [len(lines)])
    rec = "\n".join(lines[lo:hi])
    return tuple(int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1)) for k in ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"))


def steady_loop(body):
    """(first, last) line of the steady-state loop of a plane-marching kernel: the innermost loop that both loads and
    stores populations."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    cands = [lp for lp in loops
             if sum("global_store" in l for l in body[lp[0]:lp[1]]) >= 38 and sum("global_load" in l for l in body[lp[0]:lp[1]]) >= 38]
    return min(cands, key=lambda lp: lp[1] - lp[0])
