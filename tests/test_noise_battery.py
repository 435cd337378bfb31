"""CPU: the noise stream's distribution and independence (tests/noise_battery.py) on the oracle's fields, and the battery's
own teeth.

Every "GPU == oracle" assertion of the suite says that two restatements of one generator design agree; this file says that
the design yields 33 independent N(0, 1)-quantised numbers per site and noise index, against an exactly known null (the
level is a sum of four uniform bytes).  tests/test_gpu_noise_stream.py runs the same battery on the device's fields.

State: rho = phi = 1, alpha0 = 0, tau_f = tau_g = 1, kBT = 1e-5, where each draw's amplitude is one constant.

MEASURED (worst value / critical value; z = r sqrt(N); hist is the smallest p-value, which must stay ABOVE its critical value):

  case                                     tests  hist p            same_site   squares     neighbour   next index  next seed   periodogram
  64x64x32 seed 12345 index 0              6568   2.8e-3 / 1.5e-7   4.19 / 5.25 3.08 / 5.25 3.86 / 5.25 3.81 / 5.25 3.25 / 5.25 15.3 / 26.8
  64x64x32 seeds 12345, 12345 + 2^32       1089                                                                     3.64 / 4.91
  64x32x16 seed 777 index 5                4390   1.3e-2 / 2.3e-7   3.26 / 5.18 3.65 / 5.18 3.45 / 5.18                         14.7 / 25.0
  64x32x16 seed 778 index 5                4390   9.5e-2 / 2.3e-7   2.87 / 5.18 2.94 / 5.18 3.55 / 5.18                         15.5 / 25.0
  64x32x16 seed 779 index 5                4390   8.7e-2 / 2.3e-7   2.90 / 5.18 3.80 / 5.18 3.68 / 5.18                         13.2 / 25.0
  64x32x16 seed 780 index 5                4390   4.4e-3 / 2.3e-7   3.55 / 5.18 3.35 / 5.18 3.84 / 5.18                         12.4 / 25.0
  64x32x16 seeds 777..780, six pairs       6534                                                                     3.57 / 5.25
  96x80x48 seed 987654321 index 2^31       6568   1.3e-2 / 1.5e-7   3.34 / 5.25 3.66 / 5.25 3.80 / 5.25 4.02 / 5.25 3.30 / 5.25 14.8 / 27.8
      (next index 2^31 + 1, next seed 987654322; 8.7 s)

The periodogram's critical value is log(M / alpha) with M the DISTINCT non-zero ordinates of one draw position (k and -k
carry one value: 65539 of the 131071 at 64 x 64 x 32) and alpha the per-test level of the family, 1e-3 / 6568: 26.8.

The defective streams (64 x 64 x 32; the failing statistic and its value; every other statistic keeps the value of the first
row above or stays far inside its critical value, which the test asserts):
  draw 5 of site s = draw 4 of site s + e_x            neighbour 362
  3 % of the sites repeat draw 4 in draw 5             same_site 11.9, and the squares with them: same_site_sq 9.8
  draw 7's magnitudes rank-matched to draw 6's         same_site_sq 362 (same_site 4.26: no linear correlation)
  1 % of the levels replaced by uniform levels         hist p = 0
  next index = this index rotated by one draw          next_index 362
  rint(6 sin(2 pi 5 x / nx)) added to draw 9's levels  periodogram 57.8
"""
import numpy as np
import pytest

import noise_battery as nb

PAR = dict(kBT=1e-5, alpha0=0.0, tau_f=1.0, tau_g=1.0)
BASE = (64, 64, 32)
BATCH = (64, 32, 16)
BATCH_SEEDS, BATCH_INDEX = (777, 778, 779, 780), 5
LARGE = (96, 80, 48)                     # no power of two in y and z: 368640 sites, site indices that are no bit fields of x, y, z
LARGE_SEED, LARGE_INDEX = 987654321, 2 ** 31

_levels = {}


def oracle_levels(ob, n, seed, index):
    """The oracle's levels S[33, N] on unit densities, computed once per (n, seed, index) and left unchanged."""
    key = (n, seed, index)
    if key not in _levels:
        nx, ny, nz = n
        one = np.ones((nz, ny, nx))
        fn, gn = ob.thermal_noise(n, ob.default_params(seed=seed, **PAR), one, one, noise_index=index)
        S = nb.levels(fn, gn, nb.unit_state_amplitudes(ob.lattice_tables()[2], kBT=PAR["kBT"], tau=PAR["tau_f"]))
        S.setflags(write=False)
        _levels[key] = S
    return _levels[key]


def test_amplitudes_are_the_documented_expression(ob):
    """unit_state_amplitudes against the host stream: amplitude = moment / normal at the first site whose normal is not 0
    (level 510 is exactly 0), for every draw."""
    n = (8, 4, 2)
    one = np.ones(n[::-1])
    fn, gn = ob.thermal_noise(n, ob.default_params(seed=12345, **PAR), one, one, noise_index=3)
    amp = nb.unit_state_amplitudes(ob.lattice_tables()[2], kBT=PAR["kBT"], tau=PAR["tau_f"])
    draws = np.concatenate([fn[1:4], fn[4:19], gn[4:19]]).reshape(33, -1)
    z = np.array([ob.site_normals(12345, s, 3) for s in range(draws.shape[1])]).T
    assert np.all(np.isin(z, nb.table()))
    for k in range(33):
        s = int(np.flatnonzero(z[k])[0])
        assert abs(draws[k, s] / z[k, s] / amp[k] - 1.0) < 1e-14, k
    assert np.array_equal(nb.levels(fn, gn, amp), np.searchsorted(nb.table(), z))


def test_oracle_stream_base_case(ob):
    S = oracle_levels(ob, BASE, 12345, 0)
    stats = nb.battery(S, BASE, S_next_index=oracle_levels(ob, BASE, 12345, 1), S_other_seed=oracle_levels(ob, BASE, 12346, 0))
    thr = nb.thresholds(stats)
    assert thr["ntests"] == 34 + 528 + 528 + 3 * 1089 + 1089 + 1089 + 33 == 6568
    assert abs(thr["z"] - 5.25) < 0.005
    nb.check(stats, thr, f"oracle {BASE} seed 12345 index 0")


def test_oracle_stream_high_key_word(ob):
    """Seed 12345 + 2^32 differs from 12345 in the high word of the Philox key only."""
    stats = dict(next_seed=nb.cross_seed(oracle_levels(ob, BASE, 12345, 0), oracle_levels(ob, BASE, 12345 + 2 ** 32, 0)))
    nb.check(stats, nb.thresholds(stats), f"oracle {BASE} seeds 12345, 12345 + 2^32")


@pytest.mark.parametrize("seed", BATCH_SEEDS)
def test_oracle_stream_of_each_batch_seed(ob, seed):
    stats = nb.battery(oracle_levels(ob, BATCH, seed, BATCH_INDEX), BATCH)
    nb.check(stats, nb.thresholds(stats), f"oracle {BATCH} seed {seed} index {BATCH_INDEX}")


def test_oracle_streams_of_adjacent_seeds_are_independent(ob):
    """What BatchLBM gives its replicas (seed + r) and every ensemble average rests on: the six cross-seed matrices of the
    four streams, one family of 6 x 1089 tests."""
    stats = nb.cross_seed_pairs([oracle_levels(ob, BATCH, s, BATCH_INDEX) for s in BATCH_SEEDS])
    assert stats["next_seed"]["ntests"] == 6 * 1089
    nb.check(stats, nb.thresholds(stats), f"oracle {BATCH} seeds 777..780 index {BATCH_INDEX}, six pairs")


def test_oracle_stream_larger_case(ob):
    S = oracle_levels(ob, LARGE, LARGE_SEED, LARGE_INDEX)
    stats = nb.battery(S, LARGE, S_next_index=oracle_levels(ob, LARGE, LARGE_SEED, LARGE_INDEX + 1),
                       S_other_seed=oracle_levels(ob, LARGE, LARGE_SEED + 1, LARGE_INDEX))
    nb.check(stats, nb.thresholds(stats), f"oracle {LARGE} seed {LARGE_SEED} index 2^31")


# ---- the battery has teeth --------------------------------------------------------------------------------------------------
def _defect_neighbour(S, S1, rng):
    """Draw 5 of site s = draw 4 of site s + e_x."""
    nx, ny, nz = BASE
    D = S.copy()
    D[5] = np.roll(S[4].reshape(nz, ny, nx), -1, axis=2).ravel()
    return D, S1


def _defect_repeat(S, S1, rng):
    """3 % of the sites repeat draw 4 in draw 5."""
    D = S.copy()
    sites = rng.choice(S.shape[1], size=int(0.03 * S.shape[1]), replace=False)
    D[5, sites] = S[4, sites]
    return D, S1


def _defect_magnitudes(S, S1, rng):
    """Draw 7's magnitudes rank-matched to draw 6's, signs kept: no linear correlation, the squares move together."""
    D = S.copy()
    m6, m7 = np.abs(S[6].astype(int) - 510), np.abs(S[7].astype(int) - 510)
    rank6 = np.argsort(np.argsort(m6, kind="stable"), kind="stable")
    D[7] = 510 + np.where(S[7] >= 510, 1, -1) * np.sort(m7)[rank6]
    return D, S1


def _defect_uniform(S, S1, rng):
    """1 % of the levels replaced by uniform levels."""
    D = S.copy()
    hit = rng.random(S.shape) < 0.01
    D[hit] = rng.integers(0, nb.NLEVELS, size=int(hit.sum()))
    return D, S1


def _defect_rotated_index(S, S1, rng):
    """The next index = this index rotated by one draw."""
    return S.copy(), np.roll(S, 1, axis=0)


def _defect_plane_wave(S, S1, rng):
    """rint(6 sin(2 pi 5 x / nx)) added to the levels of draw 9: 0.04 sigma."""
    nx, ny, nz = BASE
    D = S.astype(int)
    wave = np.rint(6.0 * np.sin(2 * np.pi * 5 * np.arange(nx) / nx)).astype(int)
    D[9] = np.clip(D[9].reshape(nz, ny, nx) + wave[None, None, :], 0, nb.NLEVELS - 1).ravel()
    return D.astype(S.dtype), S1


# defect, the statistics that must fail, the statistics that must still pass (measured: the module docstring)
DEFECTS = [(_defect_neighbour, ["neighbour"], ["hist", "same_site", "same_site_sq", "next_index", "next_seed", "periodogram"]),
           (_defect_repeat, ["same_site", "same_site_sq"], ["hist", "neighbour", "next_index", "next_seed", "periodogram"]),
           (_defect_magnitudes, ["same_site_sq"], ["hist", "same_site", "neighbour", "next_index", "next_seed", "periodogram"]),
           (_defect_uniform, ["hist"], ["same_site", "same_site_sq", "neighbour", "next_index", "next_seed", "periodogram"]),
           (_defect_rotated_index, ["next_index"], ["hist", "same_site", "same_site_sq", "neighbour", "next_seed", "periodogram"]),
           (_defect_plane_wave, ["periodogram"], ["hist", "same_site", "same_site_sq", "neighbour", "next_index", "next_seed"])]


@pytest.mark.parametrize("defect,fails,passes", DEFECTS, ids=[d[0].__name__[8:] for d in DEFECTS])
def test_battery_catches(ob, defect, fails, passes):
    """Each defective stream is the oracle's levels changed with numpy; it must fail by the statistic named and by no other,
    so that a failure names its cause."""
    S, S1, S2 = (oracle_levels(ob, BASE, *si) for si in ((12345, 0), (12345, 1), (12346, 0)))
    D, D1 = defect(S, S1, np.random.default_rng(2024))
    assert D.shape == S.shape and D.min() >= 0 and D.max() < nb.NLEVELS
    stats = nb.battery(D, BASE, S_next_index=D1, S_other_seed=S2)
    thr = nb.thresholds(stats)
    v = nb.verdicts(stats, thr)
    for name, (worst, crit, ok) in v.items():
        print(f"{defect.__name__[8:]}: {name}: {worst:.4g} / critical {crit:.4g} {'passes' if ok else 'FAILS'}")
    assert sorted(fails + passes) == sorted(v)
    assert [name for name in v if not v[name][2]] == [name for name in v if name in fails]
    with pytest.raises(AssertionError, match=fails[0]):
        nb.check(stats, thr, defect.__name__)


def test_levels_refuses_a_field_that_is_not_on_the_table(ob):
    n = (8, 8, 4)
    one = np.ones(n[::-1])
    fn, gn = ob.thermal_noise(n, ob.default_params(seed=12345, **PAR), one, one, noise_index=0)
    amp = nb.unit_state_amplitudes(ob.lattice_tables()[2], kBT=PAR["kBT"], tau=PAR["tau_f"])
    nb.levels(fn, gn, amp)
    for arr, mode, k in ((fn, 7, 6), (gn, 18, 32)):
        bad = arr.copy()
        bad[mode, 1, 2, 3] += 1e-6 * amp[k]                              # one sample, 1e-6 of its amplitude
        with pytest.raises(AssertionError, match=f"draw {k}, site {(1 * 8 + 2) * 8 + 3}"):
            nb.levels(*((bad, gn) if arr is fn else (fn, bad)), amp)
    bad = gn.copy()
    bad[2, 0, 0, 0] = -bad[2, 0, 0, 0] if bad[2, 0, 0, 0] else 1e-9
    with pytest.raises(AssertionError, match="negatives"):
        nb.levels(fn, bad, amp)
