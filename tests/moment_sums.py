"""What the moment-trace tests share (tests/test_moment_abi.py, tests/test_gpu_moment.py): the moment matrix as integers,
written from the polynomials in the velocities (it shares no construction with analysis.moments_of, which adds and subtracts
populations in the order of the step's own transform), the record of integer populations in int64, and the integer states."""
import numpy as np

CX = [0, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1, 0, 0, 0, 0, 1, -1, 1, -1]
CY = [0, 0, 0, 1, -1, 0, 0, 1, -1, -1, 1, 1, -1, 1, -1, 0, 0, 0, 0]
CZ = [0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, 1, -1, -1, 1, 1, -1, -1, 1]
MODES, WORDS = 19, 95


def moment_matrix():
    """M[a, i] int64: moment a of population i, the 19 polynomials of the D3Q19 basis (Duenweg, Schiller and Ladd) in the
    velocity c_i of the reference's order."""
    m = np.zeros((MODES, MODES), dtype=np.int64)
    for i, (x, y, z) in enumerate(zip(CX, CY, CZ)):
        c2 = x * x + y * y + z * z
        m[:, i] = [1, x, y, z,
                   c2 - 1, 3 * x * x - c2, y * y - z * z, x * y, y * z, x * z,
                   (3 * c2 - 5) * x, (3 * c2 - 5) * y, (3 * c2 - 5) * z,
                   (y * y - z * z) * x, (z * z - x * x) * y, (x * x - y * y) * z,
                   3 * c2 * c2 - 6 * c2 + 1, (2 * c2 - 3) * (3 * x * x - c2), (2 * c2 - 3) * (y * y - z * z)]
    return m


def integer_populations(shape_zyx, seed):
    """(f, g)[19, nz, ny, nx] doubles, every entry an integer in 1..8."""
    rng = np.random.default_rng(seed)
    f = rng.integers(1, 9, size=(MODES,) + tuple(shape_zyx))
    g = rng.integers(1, 9, size=(MODES,) + tuple(shape_zyx))
    return f.astype(np.float64), g.astype(np.float64)


def integer_record(f, g):
    """The 95 words of a sample of integer populations in int64: 95 dot products over the sites.  With populations in
    1..8 a moment is below 2^9, a square below 2^18 and a box sum of 2^20 sites below 2^38: exact in doubles in any order."""
    fi, gi = np.asarray(f).astype(np.int64), np.asarray(g).astype(np.int64)
    assert np.array_equal(fi, f) and np.array_equal(gi, g)
    m = moment_matrix()
    mf = (m @ fi.reshape(MODES, -1))
    mg = (m @ gi.reshape(MODES, -1))
    return np.concatenate([mf.sum(axis=1), mg.sum(axis=1), (mf * mf).sum(axis=1), (mg * mg).sum(axis=1), (mf * mg).sum(axis=1)])


def words_of_population(fluid, i):
    """The words of a sample that population i of one fluid enters: sum, sq and cross of every mode with a non-zero
    matrix entry."""
    modes = np.nonzero(moment_matrix()[:, i])[0]
    return sorted([MODES * fluid + a for a in modes] + [MODES * (2 + fluid) + a for a in modes] + [4 * MODES + a for a in modes])
