"""Morphology traces: the cubes, faces, edges and vertices of a set of voxels by an independent construction, the closed
forms and what bflbm_morph_geometry reports (include/bflbm.h, "Morphology traces": the rule is stated there).  In the
style of hist_counts.py.

    brute(occ)                      (N3, N2, N1, N0) of occ[nz, ny, nx] from the SETS of the elements of every occupied
                                    closed voxel, coordinates modulo the box: no OR over neighbourhoods anywhere
    functionals(counts)             (V, S, 2B, chi) in Python integers
    cuboid(a, b, c)                 the closed form of an a x b x c cuboid that does not wrap: (abc, 2(ab+bc+ca), a+b+c, 1)
    projections(occ)                the three projected areas of a set: S = 2 x their sum for an orthogonally convex set
    orthogonally_convex(occ)        every line along an axis meets the set in one run at the most (no wrap)
    geometry(n, nlevels, nrep)      the launch shape of the counting kernel
"""
import numpy as np

TILE = 1024                        # plane sites of a work item
MIN_CHUNK, MAX_CHUNK = 8, 64       # planes of a work item
WANT_ITEMS = 1024                  # work items over all replicas that the chunk is shortened for


def brute(occ):
    """A voxel at (z, y, x) has the vertices (z + dz, y + dy, x + dx), d in {0, 1}; an edge is (axis, its lower vertex),
    a face (normal axis, its lower vertex); everything modulo the box, so what two voxels share, across the periodic
    planes too, is one element of the set."""
    occ = np.asarray(occ, dtype=bool)
    n = occ.shape
    cubes, faces, edges, vertices = set(), set(), set(), set()

    def at(z, y, x):
        return (z % n[0], y % n[1], x % n[2])

    for z, y, x in zip(*np.nonzero(occ)):
        z, y, x = int(z), int(y), int(x)
        cubes.add((z, y, x))
        for a in range(3):                                 # the two faces normal to axis a
            for d in (0, 1):
                s = [z, y, x]
                s[a] += d
                faces.add((a,) + at(*s))
        for a in range(3):                                 # the four edges along axis a
            b, c = [k for k in range(3) if k != a]
            for db in (0, 1):
                for dc in (0, 1):
                    s = [z, y, x]
                    s[b] += db
                    s[c] += dc
                    edges.add((a,) + at(*s))
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    vertices.add(at(z + dz, y + dy, x + dx))
    return (len(cubes), len(faces), len(edges), len(vertices))


def functionals(counts):
    n3, n2, n1, n0 = (int(v) for v in counts)
    return (n3, -6 * n3 + 2 * n2, 3 * n3 - 2 * n2 + n1, -n3 + n2 - n1 + n0)


def cuboid(a, b, c):
    return (a * b * c, 2 * (a * b + b * c + c * a), a + b + c, 1)


def projections(occ):
    occ = np.asarray(occ, dtype=bool)
    return tuple(int(occ.any(axis=a).sum()) for a in range(3))


def orthogonally_convex(occ):
    """Every lattice line along an axis meets the set in at most one run of consecutive sites, none across the wrap."""
    occ = np.asarray(occ, dtype=bool)
    for a in range(3):
        m = np.moveaxis(occ, a, -1).astype(np.int8)
        starts = (np.diff(m, axis=-1, prepend=0) == 1).sum(axis=-1)
        if (starts > 1).any():
            return False
    return True


def chunk(plane, nz, nrep=1):
    tiles = (plane + TILE - 1) // TILE
    zc = MAX_CHUNK
    while zc > MIN_CHUNK and tiles * ((nz + zc - 1) // zc) * nrep < WANT_ITEMS:
        zc //= 2
    return min(zc, nz)


def geometry(n, nlevels, nrep=1):
    """What MorphologyTrace.geometry() returns for the box n = (nx, ny, nz)."""
    plane = n[0] * n[1]
    zc = chunk(plane, n[2], nrep)
    items = ((plane + TILE - 1) // TILE) * ((n[2] + zc - 1) // zc)
    return (nlevels, TILE, zc, items, items * nrep)
