"""Cluster traces: the connected components of a set of voxels by an independent construction, the record made from them
and what bflbm_cluster_geometry reports (include/bflbm.h, "Cluster traces": the rule is stated there).  In the style of
morph_counts.py.

    neighbours(shape, connectivity) [nsites, 6 or 26] the linear indices of every site's periodic neighbours, explicit lists
    flood(occ, connectivity)        labels[nz, ny, nx] int32 by a breadth-first flood fill over those lists, sites scanned
                                    in ascending p so that the first site met of a component is its smallest: no minimum
                                    is ever propagated
    record(labels)                  the 38 words of a level in Python integers
    canonical(labels)               the set of the components as frozensets of coordinates, for comparisons under shifts
    bricks_of(labels, label)        the bricks a component has sites in
    wrapped_axes(labels, label, connectivity)   the axes along which the component contains a link across the periodic plane
    geometry(n, nlevels, connectivity)          what ClusterTrace.geometry() returns for the box n = (nx, ny, nz)
    snake(shape)                    a one-voxel-wide path through the box whose smallest site is one of its ends
"""
from collections import deque

import numpy as np

WORDS = 38
BRICK = (32, 4, 4)                 # the brick's extents along x, y, z
LAUNCHES = 4                       # per level
CONNECTIVITIES = (6, 26)


def offsets(connectivity):
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) != (0, 0, 0) and (connectivity == 26 or abs(dz) + abs(dy) + abs(dx) == 1)]


def neighbours(shape, connectivity):
    nz, ny, nx = shape
    z, y, x = np.indices(shape)
    cols = [(((z + dz) % nz) * ny + (y + dy) % ny) * nx + (x + dx) % nx for dz, dy, dx in offsets(connectivity)]
    return np.stack([c.ravel() for c in cols], axis=1)


def flood(occ, connectivity):
    occ = np.asarray(occ, dtype=bool)
    nb = neighbours(occ.shape, connectivity).tolist()
    flat = occ.ravel().tolist()
    labels = [-1] * len(flat)
    for p0 in range(len(flat)):
        if not flat[p0] or labels[p0] >= 0:
            continue
        labels[p0] = p0
        queue = deque([p0])
        while queue:
            p = queue.popleft()
            for q in nb[p]:
                if flat[q] and labels[q] < 0:
                    labels[q] = p0
                    queue.append(q)
    return np.array(labels, dtype=np.int32).reshape(occ.shape)


def record(labels):
    sizes = {}
    for v in np.asarray(labels).ravel().tolist():
        if v >= 0:
            sizes[v] = sizes.get(v, 0) + 1
    rec = [0] * WORDS
    rec[0], rec[1], rec[3] = len(sizes), sum(sizes.values()), -1
    for label in sorted(sizes):
        s = sizes[label]
        if s > rec[2]:
            rec[2], rec[3] = s, label
        rec[4] += s * s
        rec[6 + s.bit_length() - 1] += 1
    return rec


def canonical(labels):
    labels = np.asarray(labels)
    groups = {}
    for z, y, x in zip(*np.nonzero(labels >= 0)):
        groups.setdefault(int(labels[z, y, x]), []).append((int(z), int(y), int(x)))
    return groups


def bricks_of(labels, label):
    z, y, x = np.nonzero(np.asarray(labels) == label)
    return set(zip((x // BRICK[0]).tolist(), (y // BRICK[1]).tolist(), (z // BRICK[2]).tolist()))


def wrapped_axes(labels, label, connectivity):
    """The axes (0 z, 1 y, 2 x) along which two sites of the component are linked across the periodic plane."""
    inside = np.asarray(labels) == label
    out = set()
    for d in offsets(connectivity):
        for axis in range(3):
            if d[axis] != 1 or inside.shape[axis] < 2:
                continue
            moved = np.roll(inside, [-v for v in d], axis=(0, 1, 2))        # moved[s] = inside[s + d]
            last = [slice(None)] * 3
            last[axis] = slice(inside.shape[axis] - 1, None)                # the sites whose + neighbour wraps
            if (inside[tuple(last)] & moved[tuple(last)]).any():
                out.add(axis)
    return out


def bricks(n):
    return -(-n[0] // BRICK[0]) * -(-n[1] // BRICK[1]) * -(-n[2] // BRICK[2])


def geometry(n, nlevels, connectivity):
    return (nlevels, connectivity) + BRICK + (bricks(n), LAUNCHES)


def snake(shape):
    """occ[nz, ny, nx]: a boustrophedon path one voxel wide along x through every second row of every second plane, joined
    at the row ends and the plane ends, clear of the periodic planes where the extents allow: one component under both
    connectivities whose smallest site is its first."""
    nz, ny, nx = shape
    occ = np.zeros(shape, dtype=bool)
    planes = list(range(0, nz - 1, 2)) or [0]
    rows = list(range(0, ny - 1, 2)) or [0]
    x_hi = max(nx - 2, 0)
    right, y_up = True, True
    for zi, z in enumerate(planes):
        order = rows if y_up else rows[::-1]
        for yi, y in enumerate(order):
            occ[z, y, 0:x_hi + 1] = True
            if yi + 1 < len(order):                        # the joint to the next row, at the end the path has reached
                step = 1 if y_up else -1
                occ[z, y + step, x_hi if right else 0] = True
            right = not right
        if zi + 1 < len(planes):                           # the joint to the next plane, at the row the path has reached
            occ[z + 1, order[-1], 0 if right else x_hi] = True
        y_up = not y_up
    return occ
