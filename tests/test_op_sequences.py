"""The operation-sequence harness (tests/op_sequences.py) held to account on the CPU, the oracle on both sides:

  * pair coverage: over a kind's committed seeds every legal ordered pair of operation kinds is consecutive somewhere;
  * conditioning: beside every sequence runs a twin whose initial and uploaded populations differ by -1, 0 or +1 ulp
    (tolerances.one_ulp_response), re-drawn after every check; at every check the twin is within a TENTH of the two
    hand-over figures (1e-14 on the populations, 1e-13 in tolerances.check) and nothing is NaN or Inf.  That, not a
    measurement of the kernels, is what entitles tests/test_gpu_op_sequences.py to 1e-13 / 1e-12;
  * teeth: four mutants of the oracle adapter, each a few lines, are each caught by a sequence of every owner kind;
  * the unmutated adapter passes every sequence bit for bit;
  * sequence(kind, seed) is pinned by a digest.
"""
import numpy as np
import pytest

import op_sequences as ops

KINDS = sorted(ops.OWNERS)
CASES = [(k, s) for k in KINDS for s in ops.SEEDS[k]]
IDS = [f"{k}-{s}" for k, s in CASES]

DIGESTS = {
    "batch-0": "f18b6cd6daa9e14c", "batch-1": "76ce1e79d7e7635c", "batch-2": "66f15a103ba1c50b", "batch-3": "c5e4d1ebf46aa892", "batch-4": "a9f508c2ca0f4615", "batch-5": "f5ab84030bde0a67",
    "lone_exact-6": "c85c2d363f7057af", "lone_exact-1": "5f6fc0727da6e7ba", "lone_exact-2": "8d5dd02de5d51eea", "lone_exact-3": "c5075a782d19deec", "lone_exact-4": "9bb5828147c2e1eb", "lone_exact-5": "2b75eafc9f7dc6f3",
    "lone_full-0": "c7c5e3d3e56c8357", "lone_full-1": "dda9517a3bbc3783", "lone_full-8": "3e8c05d92469176e", "lone_full-9": "e86b9f2650620818", "lone_full-4": "a38708e71b758221", "lone_full-5": "b871a3a06c6c6632",
    "lone_one_tile-0": "149fb7545e77a03f", "lone_one_tile-1": "b6432afd1c7d7dbb", "lone_one_tile-2": "ebb0bff240ebe018", "lone_one_tile-3": "2c1d65cd29f60c9b", "lone_one_tile-4": "5e8c9b39f222fe3c", "lone_one_tile-5": "ef162156af088e5e",
    "lone_ragged-6": "6e67ffe675063809", "lone_ragged-7": "d987efdc98d6576b", "lone_ragged-2": "6d77a6009ddb0158", "lone_ragged-3": "f359744fce2acc55", "lone_ragged-4": "da5a1743f11e06c1", "lone_ragged-5": "3b94ed27ab76b547",
    "ring_exact-0": "6cae9a0ef09be4c3", "ring_exact-1": "a95b073ab503041d", "ring_exact-2": "e615d09c43ec57d5", "ring_exact-3": "de51f64e1280c453", "ring_exact-4": "91b9ba262dc2398e", "ring_exact-11": "f30e24637ff9bc5c",
    "ring_handover-0": "2d242f7e626cb380", "ring_handover-1": "407ac3d4975487ff", "ring_handover-2": "f3278c4a6bf5002a", "ring_handover-3": "b17c3578c4b5dd1b", "ring_handover-4": "bade1a220b0343cb", "ring_handover-5": "336452e450ec2f92",
}


def _model(pkg, ob, kind):
    return ops.Model(ob, kind, pkg.analysis.minkowski_counts)


def _adapter(cls, pkg, ob, kind):
    return cls(ob, kind, pkg.analysis.minkowski_counts)


# ---- pair coverage ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_every_legal_pair_of_kinds_is_consecutive_in_some_sequence(kind):
    table = ops.pair_table(kind, ops.SEEDS[kind])
    legal = ops.legal_pairs(kind)
    print(f"\n{kind}: {len(legal)} legal pairs over {len(ops.SEEDS[kind])} seeds (rows: first, columns: second; x: not legal)")
    print(ops.format_pair_table(kind, table))
    kinds = ops.OWNERS[kind]["kinds"]
    assert len(legal) == len(kinds) ** 2 - (len(kinds) - 2 if "retune" in kinds else 0)     # only retune's successor is forced
    assert set(table) <= legal, sorted(set(table) - legal)
    assert not legal - set(table), f"never consecutive: {sorted(legal - set(table))}"


@pytest.mark.parametrize("kind,seed", CASES, ids=IDS)
def test_a_sequence_is_well_formed(kind, seed):
    seq = ops.sequence(kind, seed)
    names = [o[0] for o in seq]
    assert 25 <= len(seq) <= 40
    assert names[0] == "reinit" and names[-2:] == ["step", "check"]
    assert set(names) <= set(ops.OWNERS[kind]["kinds"]) <= set(ops.ALPHABET)
    for (a, _), (b, _) in zip(seq, seq[1:]):
        assert (a, b) in ops.legal_pairs(kind)
    uploads = sum(n.startswith("upload") for n in names)     # each may raise the total density (2 at the most after an init) by 1 %
    for name, a in seq:
        if name == "params":                                 # inside handover_contract_params
            assert abs(a["alpha0"]) * 2.0 * 1.01 ** uploads <= 6.0


# ---- determinism --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,seed", CASES, ids=IDS)
def test_a_sequence_is_the_same_list_on_every_call_and_pinned(kind, seed):
    a, b = ops.sequence(kind, seed), ops.sequence(kind, seed)
    assert a == b and repr(a) == repr(b)
    assert eval(repr(a)) == a                                # what a failure prints can be pasted back
    assert ops.digest(a) == DIGESTS[f"{kind}-{seed}"], f'"{kind}-{seed}": "{ops.digest(a)}",'


# ---- the unmutated adapter ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,seed", CASES, ids=IDS)
def test_the_oracle_adapter_passes_bit_for_bit(pkg, ob, kind, seed):
    seq = ops.sequence(kind, seed)
    log = ops.run(seq, _adapter(ops.OracleAdapter, pkg, ob, kind), _model(pkg, ob, kind), (kind, seed))
    assert len(log) >= ops.OWNERS[kind].get("replicas", 1)   # the final check at least
    if not ops.handover_ok(ops.OWNERS[kind]["n"]) or ops.OWNERS[kind]["owner"] == "batch":
        assert not any(loose for _, _, loose in log)         # such owners are never entitled to the hand-over figures


@pytest.mark.parametrize("kind", [k for k in KINDS if ops.handover_ok(ops.OWNERS[k]["n"]) and ops.OWNERS[k]["owner"] != "batch"])
def test_a_hand_over_kind_requests_steps_that_read_frames_and_steps_that_must_not(kind):
    """What the sequences ask of the hand-over kernel, from the operations alone (an explicit request resolves to
    hand-over unless an injection is pending): over the seeds, second consecutive hand-over steps, and hand-over steps
    straight after a new state or a moved counter."""
    reading = fresh = 0
    for seed in ops.SEEDS[kind]:
        requested, pending, prev = "auto", False, None           # prev: what came before, "step" a hand-over step
        for name, a in ops.sequence(kind, seed):
            if name == "schedule":
                requested = a["name"]
            elif name == "inject":
                pending = a["seed"] is not None
            elif name in ("reinit", "upload_reset", "upload_keep", "retune", "counter"):
                pending = pending and name == "counter"
                prev = "new"
            elif name in ("step", "split_step"):
                for _ in range(a.get("k", 1)):
                    if requested == "handover" and not pending:
                        reading += prev == "step"
                        fresh += prev == "new"
                        prev = "step"
                    else:
                        prev = None
                    pending = False
    print(f"\n{kind}: {reading} hand-over steps that may read frames, {fresh} straight after a new state or a moved counter")
    assert reading >= 5 and fresh >= 3


def test_the_frame_rule_of_the_runner(pkg, ob):
    """Second consecutive hand-over step: the hand-over figures; a new state, a moved counter, an exact step or an
    injection between the two: bit for bit."""
    kind = "lone_full"
    head = [("reinit", {"init": "droplet"}), ("schedule", {"name": "handover"})]

    def loose_at_checks(middle):
        seq = head + middle + [("check", {})]
        return [l for _, _, l in ops.run(seq, _adapter(ops.OracleAdapter, pkg, ob, kind), _model(pkg, ob, kind), "frame rule")]

    assert loose_at_checks([("step", {"k": 1})]) == [False]
    assert loose_at_checks([("step", {"k": 2})]) == [True]
    assert loose_at_checks([("step", {"k": 1}), ("observe", {"what": "mass"}), ("step", {"k": 1})]) == [True]
    assert loose_at_checks([("step", {"k": 1}), ("check", {}), ("step", {"k": 1})]) == [False, True]
    assert loose_at_checks([("step", {"k": 1}), ("counter", {"n": 7}), ("step", {"k": 1})]) == [False]
    assert loose_at_checks([("step", {"k": 1}), ("upload_keep", {"seed": 3}), ("step", {"k": 1})]) == [False]
    assert loose_at_checks([("step", {"k": 2}), ("reinit", {"init": "stripe"}), ("step", {"k": 1})]) == [False]
    assert loose_at_checks([("step", {"k": 1}), ("inject", {"seed": 5}), ("step", {"k": 1}), ("step", {"k": 1})]) == [False]
    assert loose_at_checks([("step", {"k": 1}), ("inject", {"seed": 5}), ("step", {"k": 3})]) == [True]
    assert loose_at_checks([("step", {"k": 1}), ("schedule", {"name": "two_pass"}), ("step", {"k": 1}),
                            ("schedule", {"name": "handover"}), ("step", {"k": 1})]) == [False]


def test_a_failure_names_the_seed_the_operation_and_a_replayable_prefix(pkg, ob):
    kind, seed = "lone_exact", ops.SEEDS["lone_exact"][0]
    seq = ops.sequence(kind, seed)
    with pytest.raises(AssertionError) as e:
        ops.run(seq, _adapter(LateParams, pkg, ob, kind), _model(pkg, ob, kind), (kind, seed))
    msg = str(e.value)
    assert msg.startswith(f"('{kind}', {seed}): operation ")
    i = int(msg.split("operation ")[1].split(" ")[0])
    assert seq[i][0] == "check" and f"replay: run({seq[:i + 1]!r}" in msg


# ---- conditioning -----------------------------------------------------------------------------------------------------------

class Twin(ops.OracleAdapter):
    """The oracle with every population it is given, or makes, changed by -1, 0 or +1 ulp."""

    def __init__(self, *a):
        super().__init__(*a)
        self.rng = np.random.default_rng(1)

    def ulp(self, v):
        o = self.m.lat[v]
        o.f *= 1.0 + self.rng.integers(-1, 2, o.f.shape) * 2.0 ** -52
        o.g *= 1.0 + self.rng.integers(-1, 2, o.g.shape) * 2.0 ** -52
        self.m.derive(v)

    def reinit(self, v, init):
        super().reinit(v, init)
        self.ulp(v)

    def upload(self, v, f, g, reset):
        super().upload(v, f, g, reset)
        self.ulp(v)

    def after_check(self):                                   # the model has just taken the twin's populations
        for v in range(self.nviews):
            self.ulp(v)


@pytest.mark.parametrize("kind,seed", CASES, ids=IDS)
def test_a_one_ulp_twin_stays_within_a_tenth_of_the_hand_over_figures(pkg, ob, kind, seed):
    log = ops.run(ops.sequence(kind, seed), _adapter(Twin, pkg, ob, kind), _model(pkg, ob, kind), (kind, seed), rule="twin")
    assert log


# ---- teeth --------------------------------------------------------------------------------------------------------------------

class StaleHydrovs(ops.OracleAdapter):
    """M1: the step after a state-replacing operation collides with the hydrovs of the state before it (stale densities,
    stale frames)."""
    stale = None

    def _replacing(self, v, call):
        h = self.m.lat[v].h.copy()
        call()
        if h.any():
            self.stale = (self.stale or {})
            self.stale[v] = h

    def reinit(self, v, init):
        self._replacing(v, lambda: super(StaleHydrovs, self).reinit(v, init))

    def upload(self, v, f, g, reset):
        self._replacing(v, lambda: super(StaleHydrovs, self).upload(v, f, g, reset))

    def step(self, k):
        for v, h in (self.stale or {}).items():
            self.m.lat[v].h[...] = h
        self.stale = None
        super().step(k)


class DeafCounter(ops.OracleAdapter):
    """M2: set_steps_done is reported back but does not move the noise index."""
    off = None

    def set_counter(self, v, n):
        self.off = dict(self.off or {})
        self.off[v] = n - self.m.lat[v].steps

    def reinit(self, v, init):
        (self.off or {}).pop(v, None)
        super().reinit(v, init)

    def upload(self, v, f, g, reset):
        if reset:
            (self.off or {}).pop(v, None)
        super().upload(v, f, g, reset)

    def retune(self):
        self.off = None
        super().retune()

    def download(self, v):
        d = super().download(v)
        d["steps"] += (self.off or {}).get(v, 0)
        return d


class InjectionTwice(ops.OracleAdapter):
    """M3: an injection feeds two steps."""
    fed = None

    def step(self, k):
        for _ in range(k):
            inj = self.m.inj
            super().step(1)
            if inj is not None and inj is not self.fed:
                self.fed = inj
                self.m.inject(*inj)


class LateParams(ops.OracleAdapter):
    """M4: set_params takes effect one step late."""
    late = None

    def set_params(self, v, **kw):
        self.late = (self.late or []) + [(v, kw)]

    def step(self, k):
        super().step(1)
        for v, kw in self.late or []:
            super().set_params(v, **kw)
        self.late = None
        if k > 1:
            super().step(k - 1)


MUTANTS = {"M1-stale-hydrovs": StaleHydrovs, "M2-deaf-counter": DeafCounter, "M3-injection-twice": InjectionTwice, "M4-late-params": LateParams}


@pytest.mark.parametrize("mutant,kind", [(m, k) for m in sorted(MUTANTS) for k in KINDS
                                         if not m.startswith("M3") or "inject" in ops.OWNERS[k]["kinds"]])   # M3 needs an injection
def test_a_mutant_is_caught_by_a_sequence_of_every_kind_it_applies_to(pkg, ob, mutant, kind):
    caught = []
    for seed in ops.SEEDS[kind]:
        try:
            ops.run(ops.sequence(kind, seed), _adapter(MUTANTS[mutant], pkg, ob, kind), _model(pkg, ob, kind), (kind, seed))
        except AssertionError as e:
            caught.append((seed, str(e).split("\n")[0][:160]))
            break
    print(f"\n{mutant} on {kind}: " + (f"caught by seed {caught[0][0]}: {caught[0][1]}" if caught else "NOT caught"))
    assert caught, f"{mutant} passes every sequence of {kind}: seeds {ops.SEEDS[kind]}"
