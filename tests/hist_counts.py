"""Histogram traces: the binning rule written out site by site in Python floats, the layout of a sample and what
bflbm_hist_geometry reports (include/bflbm.h, "Histogram traces": the rule and the layout are stated there).  In the
style of profile_sums.py.

    blocks(nbins, pairs)                   (C, [(offset, length)]): the variables, then the pairs
    brute(fields, lo, hi, nbins, pairs)    counts[C] by a loop over the sites, one Python float operation at a time
    planted(lo, hi)                        the values every definition test plants: the edges, the signed zero, the
                                           infinities and NaN
    groups(sites, nrep), lds_counters(C)   the launch shape of the counting kernel
"""
import math

import numpy as np

TILE = 2048                        # sites of a work item
GROUPS = 512                       # workgroups of a counting launch over all replicas
MAX_TILES_PER_GROUP = 1 << 20      # x TILE = 2^31 sites: a 32-bit counter cannot wrap
SMALL_COUNTERS, MAX_COUNTERS = 4096, 16384


def blocks(nbins, pairs=()):
    lengths = [n + 3 for n in nbins] + [nbins[a] * nbins[b] + 1 for a, b in pairs]
    out, at = [], 0
    for n in lengths:
        out.append((at, n))
        at += n
    return at, out


def groups(sites, nrep=1):
    tiles = (sites + TILE - 1) // TILE
    return max(min(tiles, max(1, GROUPS // nrep)), (tiles + MAX_TILES_PER_GROUP - 1) // MAX_TILES_PER_GROUP)


def lds_counters(C):
    return SMALL_COUNTERS if C <= SMALL_COUNTERS else MAX_COUNTERS


def geometry(n, nbins, pairs=(), nrep=1):
    """What HistogramTrace.geometry() returns for the box n = (nx, ny, nz)."""
    C, blk = blocks(nbins, pairs)
    return (C, blk, TILE, groups(n[0] * n[1] * n[2], nrep), lds_counters(C))


def _bin(x, lo, scale, nbins):
    t = (x - lo) * scale
    if t != t:
        return nbins + 2
    if t < 0.0:
        return nbins
    if t >= float(nbins):
        return nbins + 1
    return int(t)


def brute(fields, lo, hi, nbins, pairs=()):
    """int64 [C]: fields[nvars, ...] binned site by site in Python floats (IEEE doubles, no contraction)."""
    x = np.asarray(fields, dtype=np.float64)
    nv = len(x)
    cols = [x[v].reshape(-1).tolist() for v in range(nv)]
    scale = [float(nbins[v]) / (float(hi[v]) - float(lo[v])) for v in range(nv)]
    C, blk = blocks(nbins, pairs)
    out = [0] * C
    for s in range(len(cols[0])):
        idx = [_bin(cols[v][s], float(lo[v]), scale[v], nbins[v]) for v in range(nv)]
        for v in range(nv):
            out[blk[v][0] + idx[v]] += 1
        for p, (a, b) in enumerate(pairs):
            off, n = blk[nv + p]
            if idx[a] < nbins[a] and idx[b] < nbins[b]:
                out[off + idx[a] * nbins[b] + idx[b]] += 1
            else:
                out[off + n - 1] += 1
    return np.array(out, dtype=np.int64)


def planted(lo, hi):
    """lo (bin 0), hi (above), the double just under hi, -0.0, +inf (above), -inf (below), NaN (nan)."""
    return [lo, hi, math.nextafter(hi, -math.inf), -0.0, math.inf, -math.inf, math.nan]


def block_sums(counts, blk):
    """[..., nblocks]: the sum of every block of counts[..., C]."""
    return np.stack([counts[..., off:off + n].sum(axis=-1) for off, n in blk], axis=-1)
