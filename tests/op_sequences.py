"""Operation sequences: seeded lists of public calls applied to an owner (a lone lattice, a ring, a batch) and mirrored
on oracle_binding.OracleLattice.  Test infrastructure, importable without a GPU.

What the library keeps between calls (the current buffer, the hand-over frames and their signatures, the validity of the
densities and of the centre of mass, a pending injection, the step counter that is the noise index, the schedule `auto`
resolves to) is reset by a handful of transitions; a mistake there gives a wrong result without an error.  The tests
that compare kernels with the oracle share one call order (create, init, step, download).  Here the ORDER is what is
drawn: `sequence(kind, seed)` is a list of operations of ALPHABET, `run` applies it to a device adapter and to `Model`
and compares at the `check` operations only, so that every other pair of kinds meets with no download between them.

The model implements include/bflbm.h, not the library: the pending injection is dropped by a new resident state and
kept by a moved counter, observables of a state with a pending injection are computed with it, the noise index is the
counter modulo 2^32.

Comparison at a check.  The runner knows from bflbm_resolved_schedule, read before every step, whether a hand-over step
ran since the last re-synchronisation that could read frames: a second consecutive hand-over step with no new state and
no moved counter between the two (the rule of handover_launch, csrc/bflbm_handover.h; the geometry clause is ignored,
which only widens "could").  If none did, every array is equal bit for bit.  If one did, the schedule's own figures
hold: populations to POP_ATOL (tests/test_gpu_unit_rate.py), hydrovs and hydrovsbar under tolerances.check(..., HYDRO_TOL),
the counter equal, the noise equal bit for bit at every site whose densities are.
"""
import hashlib

import numpy as np

import tolerances

ALPHABET = ("step", "split_step", "schedule", "params", "reinit", "upload_reset", "upload_keep", "counter", "inject",
            "observe", "exchange", "retune", "check")
_LONE = tuple(k for k in ALPHABET if k != "exchange")
_RING = ("step", "schedule", "params", "reinit", "upload_reset", "counter", "observe", "exchange", "check")
_BATCH = ("step", "schedule", "params", "reinit", "upload_reset", "upload_keep", "counter", "observe", "check")

# the smallest lattices on which each kernel family still has all its roles
OWNERS = {
    "lone_exact":    dict(owner="lone", n=(70, 9, 8), kinds=_LONE),        # ny % 4 == 1: never hand-over; padded rows
    "lone_full":     dict(owner="lone", n=(128, 8, 16), kinds=_LONE),      # two full tiles in x and in y
    "lone_one_tile": dict(owner="lone", n=(64, 4, 10), kinds=_LONE),       # every neighbour tile is the tile itself
    "lone_ragged":   dict(owner="lone", n=(130, 10, 12), kinds=_LONE),     # last tile column 2 lanes, last tile row 2 rows
    "ring_handover": dict(owner="ring", n=(128, 8, 24), kinds=_RING, nslabs=(2, 3)),   # seed even: 2 slabs, odd: 3
    "ring_exact":    dict(owner="ring", n=(70, 9, 13), kinds=_RING, nslabs=(3,)),      # unequal slabs
    "batch":         dict(owner="batch", n=(34, 9, 7), kinds=_BATCH, replicas=3),
}

STEP_COUNTS = (1, 2, 3, 5)
TAUS = ((0.5, 0.5), (1.0, 1.0), (0.8, 0.6), (0.5, 0.8))      # cross the unit-rate dispatch
ALPHA0 = (0.0, 1.5, 2.5)                                     # x total density (at most 2 x 1.01^k) stays below 6
KAPPA = (1.0, 4.0)
KBT = (0.0, 1e-5)                                            # cross MODE 0 / 1
COUNTERS = (0, 7, 1000, 2 ** 31 - 1, 2 ** 32 - 2)            # a later step crosses the 32-bit noise index
INITS = {"stripe": 0.5, "droplet": 0.3, "mixture": None}
OBSERVE = ("hydrovs", "hydrovsbar", "noise", "mass", "com", "morph")
MORPH_LEVELS = (0.3, 0.55, 1.0)
BASE_PARAMS = dict(tau_f=0.5, tau_g=0.5, alpha0=1.5, kappa=4.0, kBT=0.0, rho_lo=0.0, rho_hi=1.0, seed=2024)
INJECT_AMPLITUDE = 1e-6
POP_ATOL, HYDRO_TOL = 1e-13, 1e-12


def handover_ok(n):
    """csrc/bflbm_handover.h: the lattices the hand-over kernel takes."""
    return n[0] >= 64 and n[0] % 64 != 1 and n[1] >= 4 and n[1] % 4 != 1


def nslabs_of(kind, seed):
    s = OWNERS[kind].get("nslabs")
    return None if s is None else s[seed % len(s)]


# ---- sequences --------------------------------------------------------------------------------------------------------

def legal_pairs(kind):
    """Every ordered pair of kinds that may be consecutive: all of them, but `retune` is followed by a new state."""
    kinds = OWNERS[kind]["kinds"]
    return {(a, b) for a in kinds for b in kinds if a != "retune" or b in ("reinit", "upload_reset")}


def covering_walk(kind):
    """A deterministic walk over the kinds that takes every legal pair at least once: from where it stands it takes an
    untaken pair (towards the kind with the most untaken pairs left), or walks the shortest way to a kind that has one."""
    kinds = OWNERS[kind]["kinds"]
    todo = set(legal_pairs(kind))
    succ = {a: [b for b in kinds if (a, b) in todo] for a in kinds}
    walk = ["reinit"]
    while todo:
        a = walk[-1]
        fresh = [b for b in succ[a] if (a, b) in todo]
        if fresh:
            b = max(fresh, key=lambda b: (sum((b, c) in todo for c in succ[b]), -kinds.index(b)))
            todo.discard((a, b))
            walk.append(b)
            continue
        paths, seen = [[a]], {a}                     # breadth first to the nearest kind with an untaken pair
        while paths:
            p = paths.pop(0)
            if any((p[-1], c) in todo for c in succ[p[-1]]):
                for x, y in zip(p, p[1:]):
                    todo.discard((x, y))
                walk.extend(p[1:])
                break
            for c in succ[p[-1]]:
                if c not in seen:
                    seen.add(c)
                    paths.append(p + [c])
    return walk


CHUNKS = 6          # a kind's walk is cut into at least this many pieces; seed s carries piece s % chunks(kind)
CHUNK_MAX = 31


def chunks(kind):
    w = len(covering_walk(kind))
    return max(CHUNKS, -(-(w - 1) // (CHUNK_MAX - 1)))


def _seeds(kind, moved=()):
    """One seed per piece of the walk; `moved` = {seed: its replacement, congruent modulo chunks(kind)} for the seeds
    whose draw the conditioning test of tests/test_op_sequences.py turned down."""
    out = tuple(dict(moved).get(s, s) for s in range(chunks(kind)))
    assert all(s % chunks(kind) == c for c, s in enumerate(out))
    return out


def _draw(kind, what, rng):
    """One operation of kind `what` with arguments drawn from the small sets above."""
    spec = OWNERS[kind]
    view = {"view": int(rng.integers(spec["replicas"]))} if spec["owner"] == "batch" else {}
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    if what == "step":
        return (what, {"k": pick(STEP_COUNTS)})
    if what == "schedule":
        if spec["owner"] == "batch":
            return (what, {"name": pick(("two_pass", "fused", "auto"))})
        # where the hand-over kernel applies it is half of the draws: `auto` does not take it on lattices this small
        return (what, {"name": pick(("two_pass", "fused", "handover", "auto") + ("handover",) * (2 if handover_ok(spec["n"]) else 0))})
    if what == "params":
        tf, tg = pick(TAUS)
        return (what, dict(view, tau_f=tf, tau_g=tg, alpha0=pick(ALPHA0), kappa=pick(KAPPA), kBT=pick(KBT)))
    if what == "reinit":
        return (what, dict(view, init=pick(tuple(INITS))))
    if what in ("upload_reset", "upload_keep"):
        return (what, dict(view, seed=int(rng.integers(1 << 30))))
    if what == "counter":
        return (what, dict(view, n=pick(COUNTERS)))
    if what == "inject":
        return (what, {"seed": None if rng.random() < 0.25 else int(rng.integers(1 << 30))})
    if what == "observe":
        names = [o for o in OBSERVE if o != "morph" or spec["owner"] != "ring"]
        return (what, dict(view, what=pick(names)))
    if what == "exchange":
        return (what, {"transport": int(rng.integers(2)), "overlap": int(rng.integers(2))})
    return (what, {})                                # split_step, retune, check


def sequence(kind, seed):
    """The operations of (owner kind, seed): an init, a random stretch, the seed's piece of the kind's covering walk,
    a step and a check; 25 to 40 operations; the same list on every call."""
    spec = OWNERS[kind]
    rng = np.random.default_rng([seed, sorted(OWNERS).index(kind)])
    walk = covering_walk(kind)
    nch = chunks(kind)
    per = -(-(len(walk) - 1) // nch)
    c = seed % nch
    piece = walk[c * per:(c + 1) * per + 1]          # one kind shared with the next piece: the pair across the cut
    free = [k for k in spec["kinds"] if k != "retune"]
    weight = np.array([3.0 if k == "step" else 1.0 for k in free])
    nrand = max(3, 32 - len(piece))
    kinds = ["reinit", "schedule"] + [free[int(rng.choice(len(free), p=weight / weight.sum()))] for _ in range(nrand)] + piece
    if kinds[-1] == "retune":
        kinds.append("reinit")
    kinds += ["step", "check"]
    ops = [_draw(kind, k, rng) for k in kinds]
    if spec["owner"] == "batch":                     # the init the sequence starts with: one of every replica
        first = ops[0][1]["view"]
        ops = [_draw(kind, "reinit", rng) for _ in range(spec["replicas"] - 1)] + ops
        for r, op in enumerate(ops[:spec["replicas"] - 1]):
            op[1]["view"] = (first + 1 + r) % spec["replicas"]
    assert 25 <= len(ops) <= 40, len(ops)
    return ops


# the committed seed set: every piece of every kind's walk once.  A seed is replaced by the next one that carries the same
# piece where the one-ulp twin of its draw leaves a tenth of the hand-over figures (lone_exact 0, lone_full 2, lone_ragged
# 0 and 1: densities or velocities off by 1.1e-13 to 6.3e-13 in tolerances.errors at a check), or where the kind's seeds
# would otherwise let the mutant whose counter does not move the noise index pass (lone_full 3, ring_exact 5: no draw had
# a moved counter under kBT > 0 before a check); tests/test_op_sequences.py asserts both for the set as it stands
_MOVED = {"lone_exact": {0: 6}, "lone_full": {2: 8, 3: 9}, "lone_ragged": {0: 6, 1: 7}, "ring_exact": {5: 11}}
SEEDS = {kind: _seeds(kind, _MOVED.get(kind, ())) for kind in sorted(OWNERS)}


def digest(ops):
    return hashlib.sha256(repr(ops).encode()).hexdigest()[:16]


def pair_table(kind, seeds):
    """{(a, b): how often a is followed by b over the seeds' sequences}"""
    t = {}
    for s in seeds:
        k = [o[0] for o in sequence(kind, s)]
        for p in zip(k, k[1:]):
            t[p] = t.get(p, 0) + 1
    return t


def format_pair_table(kind, table):
    kinds = OWNERS[kind]["kinds"]
    w = max(len(k) for k in kinds)
    rows = [" " * w + " " + " ".join(f"{b[:6]:>6}" for b in kinds)]
    for a in kinds:
        rows.append(f"{a:>{w}} " + " ".join(f"{table.get((a, b), 0) or ('.' if (a, b) in legal_pairs(kind) else 'x'):>6}" for b in kinds))
    return "\n".join(rows)


# ---- seeded arrays ------------------------------------------------------------------------------------------------------

def perturbed(f, g, seed):
    """The populations changed by a seeded 1 %."""
    rng = np.random.default_rng(seed)
    return (np.ascontiguousarray(f * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, f.shape))),
            np.ascontiguousarray(g * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, g.shape))))


def injected_moments(shape, seed):
    """Noise moments that conserve each fluid's mass and the total momentum, as tests/test_gpu_parity.py injects them."""
    rng = np.random.default_rng(seed)
    fn = INJECT_AMPLITUDE * rng.standard_normal(shape)
    gn = INJECT_AMPLITUDE * rng.standard_normal(shape)
    fn[0] = 0.0
    gn[0] = 0.0
    gn[1:4] = -fn[1:4]
    return fn, gn


# ---- the model ------------------------------------------------------------------------------------------------------------

class Model:
    """One OracleLattice per view (1 for a lone lattice and a ring, B for a batch) and the rules of include/bflbm.h for
    what is not a field of the reference: the pending injection (lone owners, view 0) and the counter."""

    def __init__(self, ob, kind, minkowski=None):
        spec = OWNERS[kind]
        self.ob, self.kind, self.n = ob, kind, spec["n"]
        self.nviews = spec.get("replicas", 1)
        self.lat = [ob.OracleLattice(*self.n, params=ob.default_params(**dict(BASE_PARAMS, seed=BASE_PARAMS["seed"] + v)))
                    for v in range(self.nviews)]
        self.inj = None
        self.minkowski = minkowski

    def derive(self, v):
        """densities -> noise -> hydrovs of view v for its parameters and counter; a pending injection stands in for the noise."""
        self.lat[v].refresh()
        if v == 0 and self.inj is not None:
            self.lat[v].set_noise(*self.inj)

    def one_step(self, v):
        o = self.lat[v]
        if v == 0 and self.inj is not None:
            fn, gn = self.inj
            self.inj = None                                            # an injection feeds one step
            o.timestep_injected(fn, gn)
            o.refresh()
        else:
            o.timestep()

    def step(self, k):
        for v in range(self.nviews):
            for _ in range(k):
                self.one_step(v)

    def set_params(self, v, **kw):
        for name, val in kw.items():
            setattr(self.lat[v].p, name, val)
        self.derive(v)

    def reinit(self, v, init):
        self.inj = None if v == 0 else self.inj                        # a new resident state drops a pending injection
        arg = INITS[init]
        getattr(self.lat[v], "init_" + init)(*(() if arg is None else (arg,)))

    def upload(self, v, f, g, reset):
        o = self.lat[v]
        self.inj = None if v == 0 else self.inj
        o.f[...] = f
        o.g[...] = g
        if reset:
            o.steps = 0
        self.derive(v)

    def set_counter(self, v, n):
        self.lat[v].steps = int(n)                                     # a moved counter keeps a pending injection
        self.derive(v)

    def inject(self, fn, gn):
        self.inj = None if fn is None else (fn, gn)
        self.derive(0)

    def retune(self):
        """The state is gone and the counter 0; the arrays stay as the base of the upload that may follow."""
        self.inj = None
        self.lat[0].steps = 0

    def resync(self, v, f, g):
        o = self.lat[v]
        o.f[...] = f
        o.g[...] = g
        self.derive(v)

    def snapshot(self, v):
        o = self.lat[v]
        return dict(f=o.f.copy(), g=o.g.copy(), h=o.h.copy(), hbar=o.hbar[:9].copy(), fn=o.fn.copy(), gn=o.gn.copy(), steps=int(o.steps))

    def observe(self, what, v):
        o = self.lat[v]
        if what == "hydrovs":
            return o.h.copy()
        if what == "hydrovsbar":
            return o.hbar[:9].copy()
        if what == "noise":
            return o.fn.copy(), o.gn.copy(), o.hbar[:2].copy()
        if what == "mass":
            return np.array([o.hbar[0].sum(), o.hbar[1].sum()])
        if what == "com":
            return o.com()
        raise ValueError(what)


class OracleAdapter:
    """An OracleLattice that looks like a device owner: what the CPU tests run `run` against, and the base of the mutants.
    `auto` resolves to the exact schedule of the header; an explicit hand-over request to hand-over where the header says
    it applies, so the runner's frame rule is exercised (the oracle's doubles are the exact ones whatever is resolved)."""

    def __init__(self, ob, kind, minkowski=None):
        self.m = Model(ob, kind, minkowski)
        self.nviews, self.n, self.owner = self.m.nviews, self.m.n, OWNERS[kind]["owner"]
        self.requested = "auto"
        self.samples = []

    def close(self):
        pass

    def resolved_schedules(self):
        noisy = self.m.lat[0].p.kBT != 0.0 or self.m.inj is not None
        exact = "two_pass" if noisy else "fused"
        if self.requested == "handover":
            r = "handover" if handover_ok(self.n) and self.m.inj is None else exact
        else:
            r = exact if self.requested == "auto" else self.requested
        return [r] * (self.nviews + (self.owner == "batch"))

    def set_schedule(self, name):
        self.requested = name

    def step(self, k):
        self.m.step(k)

    def split_step(self):
        self.step(1)

    def set_params(self, v, **kw):
        self.m.set_params(v, **kw)

    def reinit(self, v, init):
        self.m.reinit(v, init)

    def upload(self, v, f, g, reset):
        self.m.upload(v, f, g, reset)

    def set_counter(self, v, n):
        self.m.set_counter(v, n)

    def inject(self, fn, gn):
        self.m.inject(fn, gn)

    def exchange(self, transport, overlap):
        pass

    def retune(self):
        self.m.retune()

    def observe(self, what, v):
        if what == "morph":
            fields = [self.m.lat[r].h[0].copy() for r in range(self.nviews)]
            self.samples.append(np.stack([self.m.minkowski(f, MORPH_LEVELS) for f in fields]))
            return len(self.samples) - 1, fields
        return self.m.observe(what, v)

    def morph_counts(self):
        return np.stack(self.samples) if self.samples else np.zeros((0, self.nviews, len(MORPH_LEVELS), 4), dtype=np.int64)

    def download(self, v):
        return self.m.snapshot(v)


# ---- the runner ---------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    assert np.array_equal(a, b), f"{what}: differs in {int(np.sum(a != b))} of {a.size} values, max |d| = {np.nanmax(np.abs(a - b)):.3e}"


def _close(a, b, atol, what):
    d = float(np.max(np.abs(a - b)))
    assert d <= atol, f"{what}: max |d| = {d:.3e} > {atol:.1e}"


def _compare_fields(dev, mod, loose, what, scale=1.0, noise=True):
    """dev, mod: dicts of f, g, h, hbar, fn, gn (whichever are there).  loose: the hand-over figures x scale."""
    for k, a in dev.items():
        if k != "steps":
            assert np.isfinite(a).all(), f"{what}: {k} is not finite"
    if not loose:
        for k in dev:
            if k != "steps":
                _same(dev[k], mod[k], f"{what}: {k}")
        return
    for k in ("f", "g"):
        if k in dev:
            _close(dev[k], mod[k], POP_ATOL * scale, f"{what}: {k}")
    for k in ("h", "hbar"):
        if k in dev:
            tolerances.check(dev[k], mod[k], f"{what}: {k}", HYDRO_TOL * scale)
    if noise and "fn" in dev:
        drawn_on_equal = (dev["rho_phi"][0] == mod["rho_phi"][0]) & (dev["rho_phi"][1] == mod["rho_phi"][1])
        for k in ("fn", "gn"):
            bad = (dev[k] != mod[k]) & drawn_on_equal[None]
            assert not bad.any(), f"{what}: {k} differs at {int(bad.sum())} values whose densities are equal"


class Report(list):
    """(operation index, view, hand-over figures used) of every check made; .steps: {schedule: steps run on it}."""

    def __init__(self):
        super().__init__()
        self.steps = {}


class _Runner:
    def __init__(self, adapter, model, rule):
        self.a, self.m, self.rule = adapter, model, rule
        self.owner = OWNERS[model.kind]["owner"]
        self.requested = "auto"
        self.ho_prev = False          # the last step ran hand-over and nothing since replaced the state or moved the counter
        self.loose = False            # a hand-over step that could read frames ran since the last re-synchronisation
        self.kept = []                # observations awaiting the next check
        self.log = Report()           # what was compared and what ran, for the tests of the harness

    # -- resolution: what the header promises, asserted before every step --------------------------------------------------
    def resolved(self):
        all_ = self.a.resolved_schedules()
        r = all_[0]
        assert all(x == r for x in all_), f"the views / slabs resolve to different schedules: {all_}"
        kbt = self.m.lat[0].p.kBT
        pending = self.m.inj is not None
        exact = "two_pass" if (kbt != 0.0 or pending) else "fused"
        if self.requested in ("two_pass", "fused"):
            assert r == self.requested, f"explicit {self.requested} resolved to {r}"
        if self.requested == "handover":
            want = "handover" if handover_ok(self.m.n) and not pending else exact
            assert r == want, f"explicit handover on {self.m.n}, injection pending {pending}, kBT {kbt}: resolved to {r}, the header says {want}"
        if pending:
            assert r != "handover", "a pending injection resolved to hand-over"
        if self.requested == "auto" and kbt != 0.0:
            assert r != "fused", "auto with kBT > 0 resolved to fused"
        if self.owner == "batch" or not handover_ok(self.m.n):
            assert r != "handover", f"hand-over resolved on {self.owner} {self.m.n}"
        return r

    def ran(self, schedule):
        self.log.steps[schedule] = self.log.steps.get(schedule, 0) + 1
        if schedule == "handover":
            self.loose = self.loose or self.ho_prev
            self.ho_prev = True
        else:
            self.ho_prev = False

    def new_state(self):
        self.ho_prev = False
        if self.m.nviews == 1:
            self.loose = False        # both sides hold the same doubles again

    # -- operations ------------------------------------------------------------------------------------------------------
    def apply(self, i, kind, a):
        m, d = self.m, self.a
        v = a.get("view", 0)
        if kind in ("step", "split_step"):
            k = a.get("k", 1)
            first = self.resolved()
            d.step(k) if kind == "step" else d.split_step()
            m.step(k)
            self.ran(first)
            if k > 1:
                later = self.resolved()       # what the steps after the first ran: the injection, if any, is spent
                for _ in range(k - 1):
                    self.ran(later)
        elif kind == "schedule":
            d.set_schedule(a["name"])
            self.requested = a["name"]
        elif kind == "params":
            kw = {k: a[k] for k in ("tau_f", "tau_g", "alpha0", "kappa", "kBT")}
            for r in range(m.nviews):         # a batch's kBT moves on every replica together
                p = kw if r == v else {"kBT": a["kBT"]}
                d.set_params(r, **p)
                m.set_params(r, **p)
        elif kind == "reinit":
            d.reinit(v, a["init"])
            m.reinit(v, a["init"])
            self.new_state()
        elif kind in ("upload_reset", "upload_keep"):
            f, g = perturbed(m.lat[v].f, m.lat[v].g, a["seed"])
            d.upload(v, f, g, kind == "upload_reset")
            m.upload(v, f, g, kind == "upload_reset")
            self.new_state()
        elif kind == "counter":
            d.set_counter(v, a["n"])
            m.set_counter(v, a["n"])
            self.ho_prev = False
        elif kind == "inject":
            fn, gn = (None, None) if a["seed"] is None else injected_moments(m.lat[0].f.shape, a["seed"])
            d.inject(fn, gn)
            m.inject(fn, gn)
        elif kind == "observe":
            got = d.observe(a["what"], v)
            want = None if a["what"] == "morph" else m.observe(a["what"], v)
            self.kept.append((i, a["what"], v, got, want, self.loose))
        elif kind == "exchange":
            d.exchange(a["transport"], a["overlap"])
        elif kind == "retune":
            d.retune()
            m.retune()
            self.new_state()
        elif kind == "check":
            self.check(i)
        else:
            raise ValueError(kind)

    def observation(self, i, what, v, got, want, loose):
        tag = f"observe {what} of operation {i}, view {v}"
        if what == "morph":
            idx, fields = got
            counts = self.a.morph_counts()
            for r, f in enumerate(fields):
                _same(counts[idx, r], self.m.minkowski(f, MORPH_LEVELS), f"{tag}: replica {r}: the record against minkowski_counts of the field")
        elif what == "hydrovs":
            _compare_fields(dict(h=got), dict(h=want), loose, tag)
        elif what == "hydrovsbar":
            _compare_fields(dict(hbar=got), dict(hbar=want), loose, tag)
        elif what == "noise":
            # the device's own densities are not part of this observation: bit equality where the model is exact, else skipped
            if not loose:
                _same(got[0], want[0], tag + ": fn")
                _same(got[1], want[1], tag + ": gn")
        elif what == "mass":
            np.testing.assert_allclose(got, want, rtol=1e-13, err_msg=tag)      # tests/test_gpu_pitch.py
        elif what == "com":
            np.testing.assert_allclose(got, want, rtol=1e-12, err_msg=tag)      # tests/test_gpu_parity.py

    def check(self, i):
        twin = self.rule == "twin"
        devs = [self.a.download(v) for v in range(self.m.nviews)]
        for v, dev in enumerate(devs):
            mod = self.m.snapshot(v)
            what = f"check at operation {i}, view {v} ({'hand-over figures' if self.loose or twin else 'bit for bit'})"
            assert dev["steps"] == mod["steps"], f"{what}: the counter is {dev['steps']}, the model's {mod['steps']}"
            dev["rho_phi"], mod["rho_phi"] = dev["hbar"][:2], mod["hbar"][:2]      # what the noise was drawn on
            _compare_fields(dev, mod, self.loose or twin, what, 0.1 if twin else 1.0, noise=not twin)
            self.log.append((i, v, self.loose))
        if not twin:
            for obs in self.kept:
                self.observation(*obs)
        self.kept = []
        for v, dev in enumerate(devs):
            self.m.resync(v, dev["f"], dev["g"])
        self.loose = False
        getattr(self.a, "after_check", lambda: None)()


def run(ops, device_adapter, model, what=None, rule="device"):
    """Apply the operations to the adapter and to the model; compare at every `check`.  A failed comparison raises with
    `what` (the owner kind and the seed), the index of the failing operation and the operations up to it, to be pasted
    back into run().  rule "twin": the adapter is the model's one-ulp twin, held to a tenth of the hand-over figures at
    every check.  -> Report."""
    r = _Runner(device_adapter, model, rule)
    for i, (kind, a) in enumerate(ops):
        try:
            r.apply(i, kind, a)
        except AssertionError as e:
            raise AssertionError(f"{what}: operation {i} {ops[i]!r}: {e}\nreplay: run({ops[:i + 1]!r}, ...)") from None
    return r.log
