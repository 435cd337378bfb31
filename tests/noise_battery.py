"""Distribution and independence battery for the thermal-noise stream (csrc/bflbm_rng.h).  numpy and scipy only: no GPU,
no oracle.  The callers (tests/test_noise_battery.py on the oracle's fields, tests/test_gpu_noise_stream.py on the
device's) hand it noise moments; it never sees a generator.

Per (seed, global site, noise index) the stream yields 33 normals x = T[s]: s is the sum of the four bytes of one 32-bit
word, T the 1021-entry table of csrc/bflbm_normal_table.h.  If the words are uniform and independent, s has EXACTLY the
pmf "4-fold convolution of 256 ones / 2^32", and the 33 levels of a site, the levels of different sites, of different
noise indices and of different seeds are independent.  That null is what the statistics below test:

  hist           chi-square of the level histogram against the exact pmf, per draw position and pooled (34 p-values);
                 tail cells merged from both ends until each merged cell expects >= 5 counts
  same_site      r sqrt(N) of the normals of every pair of draw positions (528)
  same_site_sq   the same of their squares: dependence of the magnitudes without linear correlation (528)
  neighbour      r sqrt(N) between X[k](r) and X[k'](r + e), e = +x, +y, +z periodic, all k, k' (3 x 1089)
  next_index     r sqrt(N) between X[k] and X'[k'] of a second field: the next noise index (1089)
  next_seed      ... of another seed (1089 per field)
  periodogram    per draw position the largest |FFT X[k]|^2 / N over the non-zero wavevectors of the 3-D transform (33)

r is the sample correlation (sample means and standard deviations), so r sqrt(N) is asymptotically N(0, 1) under the null
for any marginal law.  A periodogram ordinate of white unit-variance data is asymptotically Exp(1) at a wavevector k != -k;
at the (at most 7) non-zero self-conjugate wavevectors the transform is real and |F|^2 / N is chi-square with ONE degree
of freedom, whose tail exp(-t / 2) is heavier than Exp(1)'s: those ordinates are halved, since P(chi2_1 / 2 > t) =
2 Phi(-sqrt(2 t)) <= exp(-t) as well.  With M distinct ordinates (k and -k carry the same value) the largest exceeds t with
probability <= M exp(-t).

thresholds(): the family-wise false-alarm probability of one data set is `family` (1e-3), split evenly over all its tests
(Bonferroni): alpha = family / ntests per test.  Critical values are scipy.stats quantiles of that alpha: two-sided normal
for the correlations, alpha itself for the chi-square p-values (scipy.stats.chi2.sf), log(M / alpha) for the periodogram.
Nothing here is tuned to a measured value; with fixed inputs the tests are deterministic, and the family level only guards
a future legitimate redesign of the stream against a false alarm.

Draw order (csrc/bflbm_rng.h): draws 0..2 = f modes 1..3 (g modes 1..3 are their exact negatives, not draws), 3..17 = f modes
4..18, 18..32 = g modes 4..18.  A site's flat index is (z ny + y) nx + x, the order of a C-contiguous (nz, ny, nx) array."""
import os
import re

import numpy as np
from scipy import stats as sps

NDRAWS = 33
NLEVELS = 1021
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(ROOT, "binary-fluctuating-lattice-boltzmann_amd", "csrc", "bflbm_normal_table.h")

_cache = {}


def table():
    """The committed 1021 levels T[s], parsed as tests/test_oracle_pins.py parses them."""
    if "T" not in _cache:
        vals = [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", open(TABLE_H).read())]
        assert len(vals) == 1024 and all(v == 0 for v in vals[NLEVELS:])
        T = np.array(vals[:NLEVELS])
        assert np.all(np.diff(T) > 0) and T[510] == 0.0
        _cache["T"] = T
    return _cache["T"]


def level_pmf():
    """P(s), s = 0..1020: the sum of four independent uniform bytes, exactly (integers below 2^32 / 2^32)."""
    if "pmf" not in _cache:
        c = np.ones(256)
        for _ in range(3):
            c = np.convolve(c, np.ones(256))
        assert c.size == NLEVELS and c.sum() == 2.0 ** 32
        _cache["pmf"] = c / 2.0 ** 32
    return _cache["pmf"]


def unit_state_amplitudes(b, kBT=1e-5, tau=1.0, cs2=1.0 / 3.0):
    """The 33 amplitudes, in draw order, of the state rho = phi = 1 with tau_f = tau_g = tau (LBM_binary.H:117, :125-126;
    the square roots of the `theory` array of tests/test_gpu_noise.py).  b: the norms of the 19 basis vectors."""
    lam = 1.0 / (tau + 0.5)
    base = 2.0 * (lam - 0.5 * lam * lam) * kBT
    ghost = [np.sqrt(base / cs2 * b[a]) for a in range(4, 19)]
    return np.array([np.sqrt(base * 0.5)] * 3 + ghost + ghost)


def levels(fn, gn, amplitudes):
    """Noise moments (19, nz, ny, nx) x 2 of a state with rho = phi = 1 -> integer levels S[33, N] in draw order.
    amplitudes: the 33 constants that multiply the normals there (unit_state_amplitudes).  Every sample must lie within
    1e-9 of a table level after division by its amplitude: the smallest level spacing is 6.5e-3 and rounding is 1e-16, so
    anything in between separates "a table level" from "not one"."""
    fn, gn = np.asarray(fn, dtype=np.float64), np.asarray(gn, dtype=np.float64)
    assert fn.shape == gn.shape and fn.shape[0] == 19 and fn.ndim == 4, (fn.shape, gn.shape)
    amplitudes = np.asarray(amplitudes, dtype=np.float64)
    assert amplitudes.shape == (NDRAWS,) and np.all(amplitudes > 0)
    assert not fn[0].any() and not gn[0].any(), "mode 0 carries no noise"
    assert np.array_equal(gn[1:4], -fn[1:4]), "g modes 1..3 are the negatives of f's, not draws of their own"
    T = table()
    mid = 0.5 * (T[1:] + T[:-1])
    n = fn[0].size
    draws = np.concatenate([fn[1:4], fn[4:19], gn[4:19]]).reshape(NDRAWS, n)
    S = np.empty((NDRAWS, n), dtype=np.int16)
    for k in range(NDRAWS):
        x = draws[k] / amplitudes[k]
        s = np.searchsorted(mid, x)
        resid = np.abs(x - T[s])
        worst = int(np.argmax(resid))
        assert resid[worst] < 1e-9, f"draw {k}, site {worst}: {x[worst]!r} is {resid[worst]:.3e} from the nearest table level {s[worst]}"
        S[k] = s
    return S


def normals(S):
    """T[S] as float64."""
    return table()[np.asarray(S, dtype=np.intp)]


def _standardised(X):
    X = X - X.mean(axis=1, keepdims=True)
    sd = X.std(axis=1, keepdims=True)
    assert np.all(sd > 0)
    return X / sd


def cross_z(Xa, Xb):
    """r sqrt(N) between every row of Xa and every row of Xb (sample correlation): [len(Xa), len(Xb)]."""
    n = Xa.shape[1]
    assert Xb.shape[1] == n
    return _standardised(Xa) @ _standardised(Xb).T / np.sqrt(n)


def cross_seed(S, S_other):
    """The next_seed statistic alone: S against one other level array or a list of them -> the stacked 33 x 33 matrices."""
    others = S_other if isinstance(S_other, (list, tuple)) else [S_other]
    X = normals(S)
    z = np.stack([cross_z(X, normals(o)) for o in others])
    return dict(kind="z", values=z, ntests=z.size)


def cross_seed_pairs(streams):
    """Every pair of a list of level arrays as ONE family: B (B - 1) / 2 matrices of 33 x 33."""
    pairs = [(a, b) for a in range(len(streams)) for b in range(a + 1, len(streams))]
    z = np.concatenate([cross_seed(streams[a], streams[b])["values"] for a, b in pairs])
    return dict(next_seed=dict(kind="z", values=z, ntests=z.size))


def _histogram_p(counts, nsamples):
    """Chi-square p-value of level counts (1021,) against the exact pmf; tail cells merged until the expectation is >= 5."""
    expect = nsamples * level_pmf()
    # the pmf rises monotonically to the centre: cells 0..lo are merged, lo the first cell with a prefix sum >= 5 whose
    # inner neighbour expects >= 5 on its own; hi likewise from the other end
    small = int(np.count_nonzero(expect[:NLEVELS // 2] < 5.0))
    lo = max(small - 1, int(np.searchsorted(np.cumsum(expect), 5.0)))
    hi = NLEVELS - 1 - lo                                             # the pmf is symmetric
    assert 0 <= lo < hi
    e = np.concatenate([[expect[:lo + 1].sum()], expect[lo + 1:hi], [expect[hi:].sum()]])
    c = np.concatenate([[counts[:lo + 1].sum()], counts[lo + 1:hi], [counts[hi:].sum()]])
    assert e.min() >= 5.0 and c.sum() == nsamples
    chi2 = ((c - e) ** 2 / e).sum()
    return float(sps.chi2.sf(chi2, e.size - 1))


def _self_conjugate(shape3):
    """Mask [nz, ny, nx] of the wavevectors with k == -k (mod n) on every axis."""
    axes = [np.array([(2 * k) % n == 0 for k in range(n)]) for n in shape3]
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


def battery(S, shape, S_next_index=None, S_other_seed=None):
    """All statistics of one data set.  S: levels [33, N]; shape = (nx, ny, nz) with N = nx ny nz; S_next_index: the levels
    of the next noise index; S_other_seed: those of another seed (or a list of them).
    -> {name: dict(kind, values, ntests[, ordinates])}, kind "p" (p-values), "z" (r sqrt(N)) or "exp" (periodogram maxima)."""
    S = np.asarray(S)
    nx, ny, nz = shape
    n = nx * ny * nz
    assert S.shape == (NDRAWS, n), (S.shape, shape)
    assert S.min() >= 0 and S.max() < NLEVELS
    X = normals(S)
    out = {}
    counts = np.stack([np.bincount(S[k], minlength=NLEVELS) for k in range(NDRAWS)])
    p = [_histogram_p(counts[k], n) for k in range(NDRAWS)] + [_histogram_p(counts.sum(axis=0), NDRAWS * n)]
    out["hist"] = dict(kind="p", values=np.array(p), ntests=NDRAWS + 1)
    iu = np.triu_indices(NDRAWS, 1)
    out["same_site"] = dict(kind="z", values=cross_z(X, X)[iu], ntests=iu[0].size)
    out["same_site_sq"] = dict(kind="z", values=cross_z(X * X, X * X)[iu], ntests=iu[0].size)
    X3 = X.reshape(NDRAWS, nz, ny, nx)
    nb = np.stack([cross_z(X, np.roll(X3, -1, axis=ax).reshape(NDRAWS, n)) for ax in (3, 2, 1)])   # X[k'](r + e): +x, +y, +z
    out["neighbour"] = dict(kind="z", values=nb, ntests=nb.size)
    if S_next_index is not None:
        z = cross_z(X, normals(S_next_index))
        out["next_index"] = dict(kind="z", values=z, ntests=z.size)
    if S_other_seed is not None:
        out["next_seed"] = cross_seed(S, S_other_seed)
    selfc = _self_conjugate((nz, ny, nx))
    scale = np.where(selfc, 0.5, 1.0) / n
    Xs = _standardised(X).reshape(NDRAWS, nz, ny, nx)
    peak = np.empty(NDRAWS)
    for k in range(NDRAWS):
        pw = np.abs(np.fft.fftn(Xs[k])) ** 2 * scale
        pw[0, 0, 0] = 0.0
        peak[k] = pw.max()
    nself = int(selfc.sum()) - 1                                      # without k = 0
    out["periodogram"] = dict(kind="exp", values=peak, ntests=NDRAWS, ordinates=(n - 1 - nself) // 2 + nself)
    return out


def thresholds(ntests, family=1e-3):
    """Bonferroni: alpha = family / ntests per test.  ntests: the number of tests of the data set, or the dict battery()
    returned (its counts are added).  -> dict(ntests, alpha, z = two-sided normal critical value, p = the smallest
    acceptable chi-square p-value); the periodogram's critical value needs its number of ordinates: periodogram_critical."""
    if isinstance(ntests, dict):
        ntests = sum(int(s["ntests"]) for s in ntests.values())
    ntests = int(ntests)
    assert ntests > 0 and 0 < family < 1
    alpha = family / ntests
    return dict(ntests=ntests, alpha=alpha, z=float(sps.norm.isf(alpha / 2)), p=alpha)


def periodogram_critical(ordinates, alpha):
    """t with ordinates * exp(-t) = alpha."""
    return float(np.log(ordinates / alpha))


def verdicts(stats, thr):
    """{name: (worst value, critical value, passed)}: for "z" the largest |z| against thr["z"], for "p" the smallest p-value
    against thr["p"], for "exp" the largest ordinate against log(ordinates / alpha)."""
    out = {}
    for name, s in stats.items():
        v = np.asarray(s["values"], dtype=np.float64)
        assert np.isfinite(v).all(), name
        if s["kind"] == "z":
            worst, crit = float(np.abs(v).max()), thr["z"]
            ok = worst < crit
        elif s["kind"] == "p":
            worst, crit = float(v.min()), thr["p"]
            ok = worst > crit
        else:
            worst, crit = float(v.max()), periodogram_critical(s["ordinates"], thr["alpha"])
            ok = worst < crit
        out[name] = (worst, crit, bool(ok))
    return out


def check(stats, thr, what=""):
    """Assert every statistic; print value / critical value per statistic.  -> verdicts(stats, thr)."""
    v = verdicts(stats, thr)
    for name, (worst, crit, ok) in v.items():
        rel = "p min" if stats[name]["kind"] == "p" else "max"
        print(f"{what}: {name} ({stats[name]['ntests']} tests of {thr['ntests']}): {rel} {worst:.4g} / critical {crit:.4g}{'' if ok else '   FAILS'}")
    failed = [name for name, (_, _, ok) in v.items() if not ok]
    assert not failed, f"{what}: {failed} fail: " + ", ".join(f"{k} {v[k][0]:.4g} against {v[k][1]:.4g}" for k in failed)
    return v
