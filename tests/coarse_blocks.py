"""The coarse trace's rule (include/bflbm.h, "Coarse traces") written out site by site in plain Python, and the launch
shape the library builds.  `walk` shares no construction with analysis.coarse_fields: no reshape, no fancy indexing, one
Python float at a time, in the header's order (per fine column of a block dz then dy from +0.0, then the columns left to
right from +0.0; a pair's product is rounded once before it is added)."""

THREADS, GROUPS = 256, 2048

# (box (nx, ny, nz), origin, extent, block): the smallest cases at which a part of the kernel can go wrong
CASES = [
    ((8, 8, 8), (0, 0, 0), (8, 8, 8), (2, 2, 2)),            # the base case
    ((10, 6, 13), (0, 0, 1), (10, 6, 12), (5, 3, 4)),        # odd sizes, b_x not a power of two, a z offset
    ((10, 6, 13), (8, 5, 11), (6, 4, 6), (3, 2, 3)),         # the seam on all three axes
    ((10, 6, 13), (0, 0, 5), (10, 6, 1), (1, 1, 1)),         # a slice: the plane itself
    ((70, 9, 16), (0, 0, 0), (70, 9, 16), (7, 3, 2)),        # a row wider than a wave
    ((258, 4, 2), (0, 0, 0), (258, 4, 2), (3, 1, 1)),        # a tile of 255 sites; the second tile holds one block
    ((260, 3, 2), (0, 0, 0), (260, 3, 2), (65, 1, 1)),       # a tile of 195 sites
    ((520, 2, 2), (0, 0, 0), (520, 2, 2), (1, 1, 1)),        # three tiles; the field itself
    ((512, 2, 2), (0, 0, 0), (512, 2, 2), (256, 2, 1)),      # the largest b_x
]


def case_id(case):
    n, o, w, b = case
    return "n%dx%dx%d-o%d.%d.%d-w%dx%dx%d-b%dx%dx%d" % (n + o + w + b)


def walk(fields, pairs, origin, extent, block):
    """sums[q][Z][Y][X] as nested lists: fields[nvars][nz][ny][nx] (anything indexable that way, e.g. ndarray.tolist()),
    pairs of variable slots, origin / extent / block as (x, y, z)."""
    nv = len(fields)
    nz, ny, nx = len(fields[0]), len(fields[0][0]), len(fields[0][0][0])
    (ox, oy, oz), (wx, wy, wz), (bx, by, bz) = origin, extent, block
    assert wx % bx == 0 and wy % by == 0 and wz % bz == 0
    out = []
    for q in range(nv + len(pairs)):
        vol_a = fields[q] if q < nv else fields[pairs[q - nv][0]]
        vol_b = None if q < nv else fields[pairs[q - nv][1]]
        vol = []
        for Z in range(wz // bz):
            plane = []
            for Y in range(wy // by):
                row = []
                for X in range(wx // bx):
                    s = 0.0
                    for dx in range(bx):
                        x = (ox + X * bx + dx) % nx
                        c = 0.0
                        for dz in range(bz):
                            z = (oz + Z * bz + dz) % nz
                            for dy in range(by):
                                y = (oy + Y * by + dy) % ny
                                term = float(vol_a[z][y][x])
                                if vol_b is not None:
                                    term = term * float(vol_b[z][y][x])
                                c = c + term
                        s = s + c
                    row.append(s)
                plane.append(row)
            vol.append(plane)
        out.append(vol)
    return out


def tile(bx):
    """The fine sites of an x-tile: whole blocks within 256 lanes."""
    return THREADS // bx * bx


def geometry(extent, block, nq, nrep=1):
    """What bflbm_coarse_geometry reports: (c_x, c_y, c_z, Q, x-tile, work items per replica, workgroups over all
    replicas)."""
    (wx, wy, wz), (bx, by, bz) = extent, block
    t = tile(bx)
    ntiles = (wx + t - 1) // t
    lanes = (min(t, wx) + 63) // 64 * 64                     # the lanes of a work item, whole waves
    share = THREADS // lanes                                 # work items a workgroup takes at a time
    items = (wz // bz) * (wy // by) * ntiles
    turns = (items + share - 1) // share
    return (wx // bx, wy // by, wz // bz, nq, t, items, min(turns, max(1, GROUPS // nrep)) * nrep)
