"""The chord trace's rule (include/bflbm.h, "Chord traces") walked site by site in plain Python, for the tests: every line
of every axis is rotated to start at an unoccupied site and its runs are counted one site at a time.  It shares no code and
no construction with analysis.chord_counts (which pairs first and last sites found by differences), so the two check each
other.  Also the launch shapes of csrc/bflbm_chord.h restated, for the GPU tests' geometry assertions."""
import numpy as np

ROWS_PER_ITEM, LINES_PER_ITEM, GROUPS, MAX_GROUP_SITES = 4, 256, 2048, 1 << 30
MAX_LENGTH, MAX_COUNTERS = 4096, 16384


def words(max_length):
    return 1 + 3 * (3 + max_length)


def line_runs(line):
    """(spanning, [lengths]) of one periodic line of booleans."""
    n = len(line)
    zero = None
    for i in range(n):
        if not line[i]:
            zero = i
            break
    if zero is None:
        return True, []
    lengths, run = [], 0
    for k in range(1, n + 1):                              # from the site after the zero round to the zero itself
        if line[(zero + k) % n]:
            run += 1
        elif run:
            lengths.append(run)
            run = 0
    return False, lengths


def lines_of(occ, axis):
    """Every line of occ[nz][ny][nx] along axis 0 x, 1 y, 2 z, as lists of booleans."""
    nz, ny, nx = occ.shape
    if axis == 0:
        return [[bool(occ[z, y, x]) for x in range(nx)] for z in range(nz) for y in range(ny)]
    if axis == 1:
        return [[bool(occ[z, y, x]) for y in range(ny)] for z in range(nz) for x in range(nx)]
    return [[bool(occ[z, y, x]) for z in range(nz)] for y in range(ny) for x in range(nx)]


def axis_runs(occ):
    """[(spanning lines, [chord lengths]) for x, y, z] of a boolean set occ[nz][ny][nx]."""
    out = []
    for axis in range(3):
        spanning, lengths = 0, []
        for line in lines_of(occ, axis):
            full, runs = line_runs(line)
            spanning += 1 if full else 0
            lengths.extend(runs)
        out.append((spanning, lengths))
    return out


def record(occ, max_length, runs=None):
    """The W words of one level for a boolean set, as a list of ints; `runs`: axis_runs(occ) where it is at hand."""
    occ = np.asarray(occ, dtype=bool)
    rec = [int(occ.sum())]
    for spanning, lengths in (axis_runs(occ) if runs is None else runs):
        h = [0] * (max_length + 1)
        long_sites = 0
        for length in lengths:
            h[min(length, max_length)] += 1
            if length >= max_length:
                long_sites += length
        rec += [len(lengths), spanning, long_sites] + h[1:]
    assert len(rec) == words(max_length)
    return rec


def groups(n, nrep=1):
    """The workgroups of the x, y and z launches over all replicas for the box n = (nx, ny, nz)."""
    nx, ny, nz = n
    out = []
    for axis in range(3):
        if axis == 0:
            lines, extent, per = ny * nz, nx, ROWS_PER_ITEM
        else:
            lines, extent, per = nx * (nz if axis == 1 else ny), (ny if axis == 1 else nz), LINES_PER_ITEM
        items = -(-lines // per)
        item_sites = min(per, lines) * extent
        per_group = max(1, MAX_GROUP_SITES // item_sites)
        out.append(max(min(items, max(1, GROUPS // nrep)), -(-items // per_group)) * nrep)
    return tuple(out)


def geometry(n, nlevels, max_length, nrep=1):
    """What bflbm_chord_geometry reports."""
    return (nlevels, max_length, words(max_length), nlevels * words(max_length)) + groups(n, nrep)
