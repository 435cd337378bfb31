"""GPU: seeded sequences of public calls on a lone lattice, a ring and a batch against the oracle (tests/op_sequences.py).

Every test creates one owner, applies one sequence of 25 to 40 operations through the public Python surface and mirrors
it on op_sequences.Model; the device is read at the `check` operations only, so every other pair of operation kinds
meets with no download (no k_pull into the scratch buffer) between its two calls.  What is compared, and why the
hand-over figures 1e-13 / 1e-12 may be used after a step that could read frames, is in tests/op_sequences.py; that the
sequences cover every pair of kinds, are well conditioned and have teeth is tests/test_op_sequences.py (CPU).
"""
import numpy as np
import pytest

import op_sequences as ops

pytestmark = pytest.mark.gpu

CASES = [(k, s) for k in sorted(ops.OWNERS) for s in ops.SEEDS[k]]


class DeviceAdapter:
    """The owner of one kind behind the calls op_sequences.run makes."""

    def __init__(self, pkg, kind, seed):
        spec = ops.OWNERS[kind]
        self.owner, n = spec["owner"], spec["n"]
        par = [dict(ops.BASE_PARAMS, seed=ops.BASE_PARAMS["seed"] + v) for v in range(spec.get("replicas", 1))]
        if self.owner == "lone":
            self.o = pkg.BinaryLBM(*n, params=pkg.default_params(**par[0]))
            self.views = [self.o]
        elif self.owner == "ring":
            self.o = pkg.RingLBM(*n, nslabs=ops.nslabs_of(kind, seed), devices=(0,), params=pkg.default_params(**par[0]))
            self.views = [self.o]
        else:
            self.o = pkg.BatchLBM(n, params=par)
            self.views = self.o.replicas
        # sampled by hand only: no step of a sequence (nor of the placement probe) reaches the every-counter
        self.trace = None if self.owner == "ring" else self.o.morphology_trace("rho", ops.MORPH_LEVELS, every=10 ** 6, capacity=64)
        self.nsamples = 0

    def close(self):
        self.o.close()

    def resolved_schedules(self):
        if self.owner == "lone":
            return [self.o.resolved_schedule()]
        if self.owner == "ring":
            return [s.resolved_schedule() for s in self.o.slabs]
        return [self.o.resolved_schedule()] + [r.resolved_schedule() for r in self.views]     # a view runs what its batch runs

    def set_schedule(self, name):
        self.o.set_schedule(name)

    def step(self, k):
        self.o.LBM_timestep(k)

    def split_step(self):
        self.o.step_boundary()
        self.o.step_interior()
        self.o.step_finish()

    def set_params(self, v, **kw):
        self.views[v].set_params(**kw)

    def reinit(self, v, init):
        arg = ops.INITS[init]
        getattr(self.views[v], "LBM_init_" + init)(*(() if arg is None else (arg,)))

    def upload(self, v, f, g, reset):
        if reset:
            self.views[v].LBM_init(f, g)
        else:
            self.views[v].upload(f, g)
            self.views[v].commit_upload(False)

    def set_counter(self, v, n):
        self.views[v].set_steps_done(n)

    def inject(self, fn, gn):
        self.o.inject_noise(fn, gn)

    def exchange(self, transport, overlap):
        self.o.set_transport(transport)
        self.o.set_overlap(overlap)

    def retune(self):
        self.o.tune_placement(2)

    def observe(self, what, v):
        t = self.views[v]
        if what == "hydrovs":
            return t.LBM_hydrovars()
        if what == "hydrovsbar":
            return t.LBM_hydrovars_density()
        if what == "noise":
            return t.thermal_noise()
        if what == "mass":
            return np.array(t.mass())
        if what == "com":
            return t.update_com()
        assert what == "morph"
        self.trace.sample()
        self.nsamples += 1
        fields = [self.o.LBM_hydrovars()[0]] if self.owner == "lone" else list(self.o.LBM_hydrovars()[:, 0])
        return self.nsamples - 1, fields

    def morph_counts(self):
        return self.trace.read()[1]

    def download(self, v):
        t = self.views[v]
        f, g = t.populations()
        fn, gn = t.thermal_noise()
        return dict(f=f, g=g, h=t.LBM_hydrovars(), hbar=t.LBM_hydrovars_density(), fn=fn, gn=gn, steps=int(t.steps_done))


@pytest.mark.parametrize("kind,seed", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_a_sequence_of_public_calls_follows_the_oracle(pkg, ob, kind, seed):
    seq = ops.sequence(kind, seed)
    dev = DeviceAdapter(pkg, kind, seed)
    try:
        log = ops.run(seq, dev, ops.Model(ob, kind, pkg.analysis.minkowski_counts), (kind, seed))
    finally:
        dev.close()
    steps = sum(a.get("k", 1) for name, a in seq if name in ("step", "split_step"))
    print(f"\n{kind} seed {seed}: {len(seq)} operations, {steps} steps, {len(log)} comparisons, "
          f"{sum(loose for _, _, loose in log)} of them under the hand-over figures; steps by schedule: {log.steps}")
    assert log
