"""Chord traces, CPU side: analysis.chord_counts against the site-by-site walk of tests/chord_runs.py (which shares no
construction with it), the three exact identities (the third against analysis.minkowski_counts), the closed forms, the
invariances, the C-ABI surface (declared, exported, bound with the header's argument lists), the null-pointer refusals
(which must fail before any device is touched), the host part of csrc/bflbm_chord.h through a stand-alone program built
with the address and undefined-behaviour sanitizers, and the compiled kernels' metadata (hipcc cross-compiles gfx950, no
GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from device_listing import device_asm, kernels   # noqa: F401  (device_asm: the listing fixture)

import chord_runs as cr
from test_profile_abi import _declared_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc")

CHORD_SYMBOLS = ["bflbm_chord_create", "bflbm_batch_chord_create", "bflbm_chord_destroy", "bflbm_chord_sample", "bflbm_chord_reset",
                 "bflbm_chord_count", "bflbm_chord_geometry", "bflbm_chord_read"]
BOXES = [(7, 9, 5), (64, 32, 3), (6, 4, 1), (2, 2, 2), (1, 3, 2), (1, 1, 1), (33, 17, 6), (70, 5, 4), (130, 3, 2)]      # (nx, ny, nz)
FILLS = [0.05, 0.3, 0.5, 0.8, 0.97, 1.0]


def _rec(pkg, occ, max_length):
    """The twin's record of a boolean set: the field is the set itself, the level one half."""
    return pkg.analysis.chord_counts(np.asarray(occ, dtype=np.float64), [0.5], "above", max_length)[0].tolist()


def _axis(pkg, rec, axis, max_length):
    """(chords, spanning, long_sites, {length: count of the non-empty bins}) of an axis block of a record."""
    b = pkg.analysis.chord_blocks(max_length)[axis]
    h = rec[b["hist"]]
    return rec[b["chords"]], rec[b["spanning"]], rec[b["long_sites"]], {l + 1: c for l, c in enumerate(h) if c}


# ---- the numpy twin against the walk, and the identities ------------------------------------------------------------------
@pytest.mark.parametrize("n", BOXES)
def test_chord_counts_against_the_walk_and_the_identities(pkg, n):
    an = pkg.analysis
    nx, ny, nz = n
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    for fill in FILLS:
        v = rng.random((nz, ny, nx))
        for side, level, occ in (("above", 1.0 - fill, v >= 1.0 - fill), ("below", fill, v < fill)):
            runs = cr.axis_runs(occ)
            mk = an.minkowski_counts(v, [level], side)[0]
            for m in (1, 4, max(n) + 1):
                got = an.chord_counts(v, [level, 2.0 if side == "above" else -1.0], side, m)
                layout = an.chord_blocks(m)
                assert got.dtype == np.int64 and got.shape == (2, layout["W"]) and layout["W"] == cr.words(m)
                assert got[0].tolist() == cr.record(occ, m, runs), (n, fill, side, m)
                assert got[1].tolist() == cr.record(np.zeros_like(occ), m)             # the empty set: nothing anywhere
                assert np.array_equal(an.chord_counts(v, [level], 0 if side == "above" else 1, m)[0], got[0])      # the side by number
                rec, total = got[0], 0
                for name, na in zip("xyz", n):
                    b = layout[name]
                    h = rec[b["hist"]]
                    assert h.sum() == rec[b["chords"]], (n, fill, side, m, name)
                    assert (np.arange(1, m) * h[:-1]).sum() + rec[b["long_sites"]] + na * rec[b["spanning"]] == rec[0], (n, fill, side, m, name)
                    total += rec[b["chords"]]
                    if m > max(n):                         # no chord reaches the last bin
                        assert rec[b["long_sites"]] == 0 and h[-1] == 0
                assert total == mk[1] - 3 * mk[0] and rec[0] == mk[0], (n, fill, side, m)
                assert 2 * total == an.minkowski_functionals(mk)[1]                    # S = 2 sum of the chords
                mean = an.chord_mean_length(rec, n)
                for k, (name, na) in enumerate(zip("xyz", n)):
                    chords = rec[layout[name]["chords"]]
                    if chords:
                        assert mean[k] == (rec[0] - na * rec[layout[name]["spanning"]]) / chords
                    else:
                        assert np.isnan(mean[k])
        if fill == 1.0:                                    # the full box: only spanning lines
            full = an.chord_counts(v, [0.0], "above", 4)[0]
            sites = nx * ny * nz
            want = [sites] + [0, sites // nx, 0, 0, 0, 0, 0] + [0, sites // ny, 0, 0, 0, 0, 0] + [0, sites // nz, 0, 0, 0, 0, 0]
            assert full.tolist() == want


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def test_closed_forms(pkg):
    n = (9, 8, 10)                                         # [nz, ny, nx]
    m = 6
    for a, b, c in ((1, 1, 1), (3, 2, 4), (8, 7, 9), (1, 5, 1), (2, 3, 7)):
        occ = np.zeros(n, dtype=bool)
        occ[1:1 + a, 0:b, 0:c] = True                      # a along z, b along y, c along x; one empty cell before the image
        rec = _rec(pkg, occ, m)
        assert rec[0] == a * b * c
        for axis, length, lines in (("x", c, a * b), ("y", b, a * c), ("z", a, b * c)):
            want_long = length * lines if length >= m else 0
            assert _axis(pkg, rec, axis, m) == (lines, 0, want_long, {min(length, m): lines}), (a, b, c, axis)
    # the full box: only spanning lines; the empty box: nothing
    full = _rec(pkg, np.ones(n, dtype=bool), m)
    assert full[0] == 720 and [_axis(pkg, full, ax, m) for ax in "xyz"] == [(0, 72, 0, {}), (0, 90, 0, {}), (0, 80, 0, {})]
    assert _rec(pkg, np.zeros(n, dtype=bool), m) == [0] * cr.words(m)
    # one voxel: one chord of length 1 per axis
    one = np.zeros(n, dtype=bool)
    one[4, 7, 0] = True
    rec = _rec(pkg, one, m)
    assert rec[0] == 1 and all(_axis(pkg, rec, ax, m) == (1, 0, 0, {1: 1}) for ax in "xyz")
    # a line occupied but for one site: one chord of length n - 1 across the seam, for every axis and every place of the site
    for axis, ax in (("x", 2), ("y", 1), ("z", 0)):
        for hole in (0, 3, n[ax] - 1):
            line = np.zeros(n, dtype=bool)
            index = [2, 2, 2]
            index[ax] = slice(None)
            line[tuple(index)] = True
            index[ax] = hole
            line[tuple(index)] = False
            rec = _rec(pkg, line, 16)
            assert _axis(pkg, rec, axis, 16) == (1, 0, 0, {n[ax] - 1: 1}), (axis, hole)
            for other in set("xyz") - {axis}:              # across: n - 1 chords of one site
                assert _axis(pkg, rec, other, 16) == (n[ax] - 1, 0, 0, {1: n[ax] - 1})
    # a periodic slab of 3 planes: spanning lines on two axes, chords of 3 on the third; also across the periodic plane
    slab = np.zeros(n, dtype=bool)
    slab[3:6] = True
    for s in (slab, np.roll(slab, 5, axis=0)):
        rec = _rec(pkg, s, m)
        assert rec[0] == 240
        assert _axis(pkg, rec, "x", m) == (0, 3 * 8, 0, {}) and _axis(pkg, rec, "y", m) == (0, 3 * 10, 0, {})
        assert _axis(pkg, rec, "z", m) == (80, 0, 0, {3: 80})
    # the last bin: chords of M sites and more, and their sites
    rod = np.zeros(n, dtype=bool)
    rod[0, 0, 1:9] = True                                  # 8 along x
    rod[5, 5, 2:8] = True                                  # 6 along x
    rod[7, 1, 4:7] = True                                  # 3 along x
    assert _axis(pkg, _rec(pkg, rod, 6), "x", 6) == (3, 0, 14, {3: 1, 6: 2})
    assert _axis(pkg, _rec(pkg, rod, 1), "x", 1) == (3, 0, 17, {1: 3})
    assert pkg.analysis.chord_mean_length(np.array(_rec(pkg, rod, 6)), (10, 8, 9)).tolist() == [17 / 3, 1.0, 1.0]
    assert np.isnan(pkg.analysis.chord_mean_length(np.array(full), (10, 8, 9))).all()


# ---- invariances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(7, 9, 5), (6, 4, 1), (2, 2, 2), (70, 5, 4)])
def test_invariance_under_periodic_shifts_and_axis_permutation(pkg, n):
    an = pkg.analysis
    nx, ny, nz = n
    rng = np.random.default_rng(5)
    v = rng.random((nz, ny, nx))
    levels, m = [0.2, 0.5, 0.9], 5
    want = an.chord_counts(v, levels, "above", m)
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 2, 5), (-1, -1, -1), (0, 0, 64)):
        assert np.array_equal(an.chord_counts(np.roll(v, shift, axis=(0, 1, 2)), levels, "above", m), want), shift
    assert np.array_equal(an.chord_counts(v[::-1, ::-1, ::-1], levels, "above", m), want)          # the mirror image
    # transposing the field's axes permutes the axis blocks: new x is old z, new z is old x, ...
    layout = an.chord_blocks(m)
    blocks = {name: slice(layout[name]["chords"], layout[name]["hist"].stop) for name in "xyz"}
    for perm, moved in (((2, 1, 0), {"x": "z", "y": "y", "z": "x"}), ((1, 0, 2), {"x": "x", "y": "z", "z": "y"}),
                        ((1, 2, 0), {"x": "z", "y": "x", "z": "y"})):
        got = an.chord_counts(v.transpose(perm), levels, "above", m)
        assert np.array_equal(got[:, 0], want[:, 0])
        for new, old in moved.items():
            assert np.array_equal(got[:, blocks[new]], want[:, blocks[old]]), (perm, new)


def test_planted_values(pkg):
    """A site equal to the level is occupied above and not below; a NaN occupies nothing on either side, so it ends the
    chords of both sides; +inf is above every finite level."""
    an = pkg.analysis
    v = np.full((1, 1, 8), 0.25)
    v[0, 0, 2:5] = 0.5
    above, below = an.chord_counts(v, [0.5], "above", 8)[0], an.chord_counts(v, [0.5], "below", 8)[0]
    assert _axis(pkg, above.tolist(), "x", 8) == (1, 0, 0, {3: 1}) and _axis(pkg, below.tolist(), "x", 8) == (1, 0, 0, {5: 1})
    assert _axis(pkg, above.tolist(), "y", 8) == (0, 3, 0, {}) and _axis(pkg, below.tolist(), "z", 8) == (0, 5, 0, {})      # extent 1: spanning
    v[0, 0, 3] = np.nan                                    # splits the run above, lengthens nothing below
    above, below = an.chord_counts(v, [0.5], "above", 8)[0], an.chord_counts(v, [0.5], "below", 8)[0]
    assert _axis(pkg, above.tolist(), "x", 8) == (2, 0, 0, {1: 2}) and _axis(pkg, below.tolist(), "x", 8) == (1, 0, 0, {5: 1})
    assert above[0] + below[0] == 7
    assert _axis(pkg, above.tolist(), "y", 8)[1] == 2 and _axis(pkg, below.tolist(), "y", 8)[1] == 5      # the NaN's own y line is not spanning
    line = np.full((1, 1, 6), np.nan)
    assert not an.chord_counts(line, [0.0], "above", 4).any() and not an.chord_counts(line, [0.0], "below", 4).any()
    v = np.zeros((1, 1, 6))
    v[0, 0, 0], v[0, 0, 5] = np.inf, np.inf
    big = np.finfo(np.float64).max
    assert _axis(pkg, an.chord_counts(v, [big], "above", 4)[0].tolist(), "x", 4) == (1, 0, 0, {2: 1})      # 5 and 0: one chord across the seam


def test_twin_refuses_bad_arguments(pkg):
    an = pkg.analysis
    f = np.zeros((3, 4, 5))
    for bad in (lambda: an.chord_counts(f[0], [0.0]), lambda: an.chord_counts(f, []), lambda: an.chord_counts(f, [0.0] * 9),
                lambda: an.chord_counts(f, [np.nan]), lambda: an.chord_counts(f, [0.0], "left"), lambda: an.chord_counts(f, [0.0], 2),
                lambda: an.chord_counts(f, [0.0], "above", 0), lambda: an.chord_counts(f, [0.0], "above", 4097),
                lambda: an.chord_counts(np.zeros((0, 4, 5)), [0.0]), lambda: an.chord_blocks(0),
                lambda: an.chord_mean_length(np.zeros((2, 14), dtype=np.int64), (3, 4, 5)), lambda: an.chord_mean_length(np.zeros((2, 13)), (3, 4, 5))):
        with pytest.raises(ValueError):
            bad()
    assert an.chord_counts(f, 0.0).shape == (1, 202) and an.chord_counts(f, [0.0] * 8, "below", 4096).shape == (8, 12298)
    assert an.CHORD_MAX_LENGTH == 4096 and an.chord_blocks(64)["z"]["hist"] == slice(138, 202)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_chord_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "bflbm.h")).read()
    lib = pkg._lib.load()
    for name in CHORD_SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        res, args = pkg._lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _declared_arguments(header, name), name
    sig = pkg._lib.SIGNATURES
    assert sig["bflbm_chord_create"] == sig["bflbm_batch_chord_create"]
    # (owner, source, var, nlevels, levels, side, max_length, every, capacity, out)
    assert len(sig["bflbm_chord_create"][1]) == 10 and sig["bflbm_chord_create"][1][8] is ctypes.c_longlong
    assert sig["bflbm_chord_read"][1][3] == ctypes.POINTER(ctypes.c_longlong)          # integers, not doubles
    assert len(sig["bflbm_chord_geometry"][1]) == 8
    assert header.count("Chord traces:") == 1 and "#define BFLBM_ABI_VERSION 1\n" in header
    assert "bflbm_ring_chord_create" not in sig and not hasattr(lib, "bflbm_ring_chord_create")      # a ring is out of scope
    assert hasattr(pkg, "ChordTrace") and "ChordTrace" in pkg.__all__
    for owner in (pkg.BinaryLBM, pkg.BatchLBM):
        assert hasattr(owner, "chord_trace")
    assert not hasattr(pkg.RingLBM, "chord_trace")
    for fn in ("chord_counts", "chord_blocks", "chord_mean_length"):
        assert hasattr(pkg.analysis, fn)
    # the header, the numpy twin and the tests' helper state the same constants
    assert pkg.analysis.CHORD_MAX_LENGTH == cr.MAX_LENGTH == 4096
    block = header[header.index("Chord traces:"):header.index("typedef struct bflbm_chord")]
    for words in ("nlevels in 1..8", "max_length M in", "1..%d" % cr.MAX_LENGTH, "W = 1 + 3 (3 + M)", "sum_l h[l] = chords",
                  "sum_{l<M} l h[l] + long_sites + n_a spanning = V", "chords_x + chords_y + chords_z = N2 - 3 N3",
                  "(V - n_a spanning) / chords", "%d counters" % cr.MAX_COUNTERS, "%d / replicas" % cr.GROUPS, "2^30 sites",
                  "no bflbm_ring_chord_create", "24 bytes per site", "No scratch", "no static LDS"):
        assert words in block, words


def test_chord_null_pointers_are_refused(pkg):
    lib = pkg._lib.load()
    h = ctypes.c_void_p()
    n, b = ctypes.c_longlong(), ctypes.c_int()
    buf = (ctypes.c_longlong * 16)()
    levels = (ctypes.c_double * 1)(0.5)
    g = [ctypes.c_int() for _ in range(7)]
    calls = {name: (lambda name=name: getattr(lib, name)(None, 0, 0, 1, levels, 0, 64, 1, 4, ctypes.byref(h))) for name in CHORD_SYMBOLS[:2]}
    calls.update({
        "bflbm_chord_sample": lambda: lib.bflbm_chord_sample(None),
        "bflbm_chord_reset": lambda: lib.bflbm_chord_reset(None),
        "bflbm_chord_count": lambda: lib.bflbm_chord_count(None, ctypes.byref(n), ctypes.byref(b)),
        "bflbm_chord_geometry": lambda: lib.bflbm_chord_geometry(None, *[ctypes.byref(x) for x in g]),
        "bflbm_chord_read": lambda: lib.bflbm_chord_read(None, 0, 1, buf, None),
    })
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.bflbm_last_error().decode()
        assert "null" in msg and name in msg, (name, msg)
        assert not h.value
    # a null level array and a null result are refused before the owner is looked at: any non-null pointer will do
    owner = ctypes.cast(buf, ctypes.c_void_p)
    for name in CHORD_SYMBOLS[:2]:
        assert getattr(lib, name)(owner, 0, 0, 1, None, 0, 64, 1, 4, ctypes.byref(h)) != 0
        assert "null" in lib.bflbm_last_error().decode() and name in lib.bflbm_last_error().decode()
        assert getattr(lib, name)(owner, 0, 0, 1, levels, 0, 64, 1, 4, None) != 0
        assert "null" in lib.bflbm_last_error().decode() and not h.value
    assert lib.bflbm_chord_destroy(None) == 0              # like every destroy of the ABI: nothing to do


# ---- the host part under the sanitizers ---------------------------------------------------------------------------------
def test_layout_launch_shapes_and_refusals_of_the_host_part(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    out = tmp_path / "chord_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "-o", str(out), os.path.join(ROOT, "tests", "chord_main.cpp")], check=True, timeout=600)
    run = subprocess.run([str(out)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.fullmatch(r"OK \d+", run.stdout.strip()), (run.stdout[-2000:], run.stderr[-3000:])
    assert int(run.stdout.split()[1]) == CHECKS


CHECKS = 31  # the checks chord_main.cpp makes: a check that silently stops running fails here


def test_the_helper_mirrors_the_launch_shape():
    """tests/chord_runs.geometry against the figures chord_main.cpp holds the host part to."""
    assert cr.geometry((7, 9, 5), 3, 64) == (3, 64, 202, 606, 12, 1, 1) and cr.geometry((34, 31, 19), 8, 4) == (8, 4, 22, 176, 148, 3, 5)
    assert cr.geometry((256, 256, 256), 3, 64) == (3, 64, 202, 606, 2048, 256, 256)
    assert cr.geometry((64, 64, 64), 3, 64, 16) == (3, 64, 202, 606, 2048, 256, 256) and cr.groups((8, 8, 8), 4096) == (4096, 4096, 4096)
    assert cr.groups((1 << 15, 1 << 15, 1 << 20))[2] == 1 << 20 and cr.groups((1, 1, 1)) == (1, 1, 1)


# ---- the compiled kernels ----------------------------------------------------------------------------------------------
def test_chord_kernel_metadata(device_asm):
    """k_chord_rows<NL> and k_chord_march<NL>, NL = 1 .. 8: no scratch in any instantiation and no static LDS, as
    include/bflbm.h states (the counters are the launch's dynamic LDS, 4 nlevels W bytes).  One marching kernel serves y
    and z.  The finishing launch is k_hist_finish, compiled once and shared."""
    for name in ("k_chord_rows", "k_chord_march"):
        found = kernels(device_asm, r"^_Z\w*?%d%sILi(\d)EE\w*:" % (len(name), name))      # Itanium mangling: <length><name>
        assert sorted(int(m.group(1)) for m, _ in found) == list(range(1, 9)), name
        for m, meta in found:
            assert re.search(r"; LDSByteSize: 0\b", meta), f"{m.group(0)}: static LDS"
            assert re.search(r"; ScratchSize: 0\b", meta), f"{m.group(0)} spills to scratch"
    assert len(kernels(device_asm, r"^_Z\w*?\d+k_chord_\w*:")) == 16                     # no third counting kernel
    assert len(kernels(device_asm, r"^_Z\w*?13k_hist_finish(E)\w*:")) == 1               # one finishing kernel, shared
