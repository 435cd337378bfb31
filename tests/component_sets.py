"""Component traces: header and rows of a level by an independent construction in Python integers from the flood-fill
labels of tests/cluster_sets.py (include/bflbm.h, "Component traces": the rule is stated there).  Nothing here is an array
operation: explicit per-component coordinate sets, the arc found by a circular scan, sums by loops, faces by explicit
neighbour lists.

    table(occ, connectivity, min_size, rows)    (header, rows, single_arc) of the boolean set occ[nz, ny, nx]: 6 integers,
                                                `rows` lists of 18 integers, and whether every component's projection
                                                on every axis was one arc (or everything)
    arcs(coords, n)                             the maximal runs of occupied coordinates on a periodic axis: (start, length)
    central(row)                                the integer central moments size sum d_a d_b - sum d_a sum d_b, 6 of them
    corner_cuboid(shape, a, b, c)               occ with an a x b x c cuboid (along x, y, z) planted across the periodic corner
    geometry(nlevels, connectivity, min_size, rows)   what ComponentTrace.geometry() returns
"""
import numpy as np

import cluster_sets as cs

HEADER, ROW, MAX_ROWS = 6, 18, 256
LAUNCHES = 9                       # per level
PAIRS = [(1, 256), (1, 4), (3, 16)]    # (min_size, rows)


def arcs(coords, n):
    """The maximal runs of the set `coords` on the periodic axis 0..n-1, found by a circular scan from an unoccupied
    coordinate: [(start, length)]; [(0, n)] where every coordinate is occupied."""
    present = set(coords)
    if len(present) == n:
        return [(0, n)]
    gap = next(c for c in range(n) if c not in present)
    runs, c = [], gap
    for _ in range(n):
        c = (c + 1) % n
        if c in present and (c - 1) % n not in present:
            length = 0
            while (c + length) % n in present:
                length += 1
            runs.append((c, length))
    return sorted(runs)


def table(occ, connectivity, min_size, rows):
    occ = np.asarray(occ, dtype=bool)
    nz, ny, nx = occ.shape
    n = (nx, ny, nz)
    labels = cs.flood(occ, connectivity)
    groups = cs.canonical(labels)                          # label -> [(z, y, x)]
    flat = occ.ravel().tolist()
    header = [len(groups), sum(len(g) for g in groups.values()), 0, 0, 0, 0]
    out, single_arc = [], True
    for label in sorted(groups):
        sites = groups[label]
        coords = ([s[2] for s in sites], [s[1] for s in sites], [s[0] for s in sites])        # x, y, z
        runs = [arcs(coords[a], n[a]) for a in range(3)]
        single_arc = single_arc and all(len(r) == 1 for r in runs)
        if len(sites) < min_size:
            continue
        header[2] += 1
        header[3] += len(sites)
        if len(out) == rows:
            continue
        origin = [r[0][0] for r in runs]
        extent = [sum(length for _, length in r) for r in runs]
        row = [label, len(sites)] + origin + extent + [0] * 10
        for z, y, x in sites:
            d = [(c - o) % m for c, o, m in zip((x, y, z), origin, n)]
            for a in range(3):
                row[8 + a] += d[a]
                row[11 + a] += d[a] * d[a]
            row[14] += d[0] * d[1]
            row[15] += d[0] * d[2]
            row[16] += d[1] * d[2]
            neighbours = [(z, y, (x + 1) % nx), (z, y, (x - 1) % nx), (z, (y + 1) % ny, x), (z, (y - 1) % ny, x),
                          ((z + 1) % nz, y, x), ((z - 1) % nz, y, x)]
            row[17] += sum(1 for (zq, yq, xq) in neighbours if not flat[(zq * ny + yq) * nx + xq])
        out.append(row)
    header[4] = len(out)
    out += [[-1] + [0] * (ROW - 1) for _ in range(rows - len(out))]
    return header, out, single_arc


def central(row):
    s = row[1]
    m1, m2, cross = row[8:11], row[11:14], row[14:17]
    return [s * m2[a] - m1[a] * m1[a] for a in range(3)] + [s * cross[0] - m1[0] * m1[1], s * cross[1] - m1[0] * m1[2], s * cross[2] - m1[1] * m1[2]]


def corner_cuboid(shape, a, b, c):
    """occ[nz, ny, nx]: the cuboid of a x b x c sites along x, y, z that starts one site before the periodic corner on
    every axis: it lies across all three periodic planes (a < nx, b < ny, c < nz asked)."""
    nz, ny, nx = shape
    assert 2 <= a < nx and 2 <= b < ny and 2 <= c < nz
    occ = np.zeros(shape, dtype=bool)
    xs, ys, zs = [(nx - 1 + i) % nx for i in range(a)], [(ny - 1 + i) % ny for i in range(b)], [(nz - 1 + i) % nz for i in range(c)]
    occ[np.ix_(zs, ys, xs)] = True
    return occ


def cuboid_row(shape, a, b, c):
    """The closed form of corner_cuboid's one row: sum d = size (a - 1) / 2, sum d^2 = size (a - 1)(2a - 1) / 6, the
    cross sums size (a - 1)(b - 1) / 4, faces 2 (ab + bc + ca); the label is site 0, which the cuboid contains."""
    nz, ny, nx = shape
    size = a * b * c
    e = (a, b, c)
    return ([0, size, nx - 1, ny - 1, nz - 1, a, b, c] + [size * (v - 1) // 2 for v in e] + [size * (v - 1) * (2 * v - 1) // 6 for v in e] +
            [size * (a - 1) * (b - 1) // 4, size * (a - 1) * (c - 1) // 4, size * (b - 1) * (c - 1) // 4, 2 * (a * b + b * c + c * a)])


def geometry(nlevels, connectivity, min_size, rows):
    return (nlevels, connectivity, min_size, rows, HEADER, ROW, LAUNCHES)
