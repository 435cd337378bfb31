"""CPU: the exact reference and the a-priori bound of tests/exact_sums.py, checked against each other without a GPU.

1. exact_moments equals a term-by-term sum in Fractions on small fields of every kind it is asked to take.
2. The device's summation order, restated in numpy (emulate_two_stage, emulate_host_blocks), stays inside depth_bound of
   the exact sum on every shape tests/test_gpu_wide_planes.py uses: the bound holds for a correct reduction.
3. The same order with stage 2 cut to its first pass (b < min(nbx, 256)) misses the bound on every shape with more than 256
   blocks per plane, for every moment, and changes nothing on the control shape: the bound separates right from wrong."""
from fractions import Fraction

import numpy as np
import pytest

import exact_sums as xs

RING_SHAPES = [(500, 135, 8), (500, 135, 13)]                           # what the ring tests decompose
SHAPES = [s for s, _, _ in xs.WIDE_SHAPES] + RING_SHAPES
_cache = {}


def _case(shape):
    """The field of a shape with its exact sums and device terms, computed once."""
    if shape not in _cache:
        rho = xs.uniform_field(shape, seed=20240 + sum(shape))
        _cache[shape] = dict(rho=rho, sets=[
            ("plain", xs.exact_moments(rho), xs.device_terms(rho)),
            ("weighted", xs.exact_moments(rho, weighted=True), xs.device_terms(rho, weighted=True)),
            ("above 1.0", xs.exact_moments(rho, threshold=1.0), xs.device_terms(rho, threshold=1.0))])
    return _cache[shape]


def _brute(rho, weighted, threshold):
    nz, ny, nx = rho.shape
    n = 10 if threshold is None else 12
    out, ab = [Fraction(0)] * n, [Fraction(0)] * n
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                r = Fraction(float(rho[z, y, x]))
                w = r
                if weighted:
                    for a, m in ((x, nx), (y, ny), (z, nz)):
                        if a == 0 or a == m - 1:
                            w /= 2
                mono = [1, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
                above = threshold is None or threshold == -np.inf or rho[z, y, x] > threshold
                terms = [w * m if above else Fraction(0) for m in mono]
                if threshold is not None:
                    terms += [r, Fraction(int(above))]
                out = [o + t for o, t in zip(out, terms)]
                ab = [o + abs(t) for o, t in zip(ab, terms)]
    return out, ab


@pytest.mark.parametrize("shape", [(5, 4, 3), (7, 1, 2), (1, 3, 1), (18, 3, 2)])
def test_exact_moments_against_fractions(shape):
    rng = np.random.default_rng(7)
    nx, ny, nz = shape
    fields = [0.5 + rng.random((nz, ny, nx)),                                          # the fields of the GPU tests
              rng.standard_normal((nz, ny, nx)) * 10.0 ** rng.integers(-12, 12, (nz, ny, nx)),   # signs, many exponents
              np.where(rng.random((nz, ny, nx)) < 0.5, 0.0, rng.random((nz, ny, nx)))]  # zeros among the sites
    for rho in fields:
        for weighted, threshold in ((False, None), (True, None), (False, 0.75), (False, -np.inf)):
            got = xs.exact_moments(rho, weighted=weighted, threshold=threshold)
            assert got == _brute(rho, weighted, threshold), (shape, weighted, threshold)
            assert all(isinstance(v, Fraction) for v in got[0] + got[1])


def test_geometry_and_depths():
    for shape, pitch, nbx in xs.WIDE_SHAPES:
        assert (xs.pitch_of(shape[0]), xs.blocks_per_plane(*shape[:2])) == (pitch, nbx)
    assert xs.pitch_of(16) == 16 and xs.pitch_of(17) == 32 and xs.pitch_of(8) == 8
    assert 1008 * 141 - 555 * 256 == 48        # the ragged last block of 1000 x 141
    u = xs.U
    for (shape, d) in (((512, 128, 3), 1 + 8 + 1 + 8 + 3), ((4112, 16, 3), 1 + 8 + 2 + 8 + 3), ((500, 135, 4), 1 + 8 + 2 + 8 + 4),
                       ((1000, 141, 2), 1 + 8 + 3 + 8 + 2)):
        assert xs.depth_bound("two_stage", *shape) == d * u / (1 - d * u)
    assert xs.depth_bound("two_stage", 500, 135, 8, nslabs=3) == xs.depth_bound("two_stage", 500, 135, 8)
    assert xs.depth_bound("host_blocks", 1000, 141, 2) == 1121 * u / (1 - 1121 * u)
    assert xs.depth_bound("host_blocks", 500, 135, 8, nslabs=3) == (9 + 270 * 3 + 3) * u / (1 - (9 + 270 * 3 + 3) * u)
    with pytest.raises(ValueError):
        xs.depth_bound("one_stage", 8, 8, 8)


@pytest.mark.parametrize("shape", SHAPES)
def test_device_order_stays_inside_the_bound(shape):
    bound = xs.depth_bound("two_stage", *shape)
    worst = 0.0
    for name, (exact, abs_sum), terms in _case(shape)["sets"]:
        for k, t in enumerate(terms):
            ratio = xs.ratio_to_bound(xs.emulate_two_stage(t), exact[k], abs_sum[k], bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (shape, name, k, ratio)
    print(f"{shape}: two_stage bound {bound:.3e}, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("shape", SHAPES)
def test_host_block_order_stays_inside_the_bound(shape):
    bound = xs.depth_bound("host_blocks", *shape)
    name, (exact, abs_sum), terms = _case(shape)["sets"][0]
    for k in range(4):                                                  # mass, x, y, z: what k_reduce adds of rho
        ratio = xs.ratio_to_bound(xs.emulate_host_blocks(terms[k]), exact[k], abs_sum[k], bound)
        assert ratio <= 1.0, (shape, k, ratio)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_truncated_second_pass_misses_the_bound(shape):
    bound = xs.depth_bound("two_stage", *shape)
    nbx = xs.blocks_per_plane(*shape[:2])
    for name, (exact, abs_sum), terms in _case(shape)["sets"]:
        for k, t in enumerate(terms):
            cut = xs.emulate_two_stage(t, first_pass_only=True)
            if nbx <= xs.BLOCK:
                assert cut == xs.emulate_two_stage(t), (shape, name, k)  # one pass serves the control: nothing is lost
            else:
                ratio = xs.ratio_to_bound(cut, exact[k], abs_sum[k], bound)
                assert ratio > 1.0, (shape, name, k, ratio)
