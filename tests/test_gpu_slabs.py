"""GPU: the z-slab path of the HIP library (halo tables, split step, upload exchange) with several
slab contexts on one GPU (slab.LocalSlabRing: same protocol as the RCCL driver, device-to-device
copies instead of sends), bit for bit against the single-box oracle; and the torch.distributed
driver itself with world_size 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    if not np.array_equal(a, b):
        raise AssertionError(f"{what}: {np.count_nonzero(a != b)} of {a.size} differ, max abs {np.abs(a - b).max():.3e}")


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("nslabs,n", [(2, (8, 8, 8)), (3, (10, 6, 13)), (4, (16, 16, 16)), (2, (70, 9, 12))])
def test_slab_ring_zero_noise(pkg, ob, nslabs, n, schedule):
    ring = pkg.LocalSlabRing(*n, nslabs, schedule=schedule)
    ref = ob.OracleLattice(*n)
    ring.LBM_init_droplet(0.3)
    ref.init_droplet(0.3)
    f, g = ring.populations()
    _same(f, ref.f, "f after init")
    for s in range(6):
        ring.LBM_timestep(1)
        ref.timestep()
    f, g = ring.populations()
    _same(f, ref.f, "f")
    _same(g, ref.g, "g")
    _same(ring.LBM_hydrovars(), ref.h, "hydrovs")
    _same(ring.LBM_hydrovars_density(), ref.hbar[:9], "hydrovsbar")
    np.testing.assert_allclose(ring.update_com(), ref.com(), rtol=1e-12)
    ring.close()


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
def test_slab_ring_with_noise_is_decomposition_independent(pkg, ob, schedule):
    """The random stream is keyed by the GLOBAL site index: 1, 2 and 4 slabs give identical bits
    (unlike AMReX's per-box stream, SURVEY 7 'RNG parity')."""
    n = (8, 8, 16)
    par = dict(kBT=1e-5, alpha0=1.5, seed=777)
    ref = ob.OracleLattice(*n, params=ob.default_params(**par))
    ref.init_stripe(0.5)
    for _ in range(4):
        ref.timestep()
    for nslabs in (1, 2, 4):
        ring = pkg.LocalSlabRing(*n, nslabs, params=pkg.default_params(**par), schedule=schedule)
        ring.LBM_init_stripe(0.5)
        ring.LBM_timestep(4)
        f, g = ring.populations()
        _same(f, ref.f, f"f with {nslabs} slabs")
        _same(g, ref.g, f"g with {nslabs} slabs")
        fn, gn = ring.thermal_noise()
        _same(fn, ref.fn, "fnoise")
        _same(gn, ref.gn, "gnoise")
        ring.close()


def test_slab_ring_upload_path(pkg, ob):
    n = (6, 7, 12)
    rng = np.random.default_rng(2)
    ref = ob.OracleLattice(*n)
    ref.init_droplet(0.3)
    f0 = ref.f * (1 + 0.01 * rng.standard_normal(ref.f.shape))
    g0 = ref.g * (1 + 0.01 * rng.standard_normal(ref.g.shape))
    ref.init_from(f0, g0)
    ring = pkg.LocalSlabRing(*n, 3)
    ring.LBM_init(f0, g0)
    f, g = ring.populations()
    _same(f, f0, "download(upload(f))")
    ring.LBM_timestep(3)
    for _ in range(3):
        ref.timestep()
    f, g = ring.populations()
    _same(f, ref.f, "f")
    _same(g, ref.g, "g")
    ring.close()


def test_slab_ring_upload_hands_every_slab_the_lattice_maximum(pkg):
    """LocalSlabRing.LBM_init: every slab resolves `auto` on the largest |rho + phi| of the whole upload, not of its own
    planes (as SlabLattice.LBM_init and bflbm_ring_commit_upload do)."""
    n = (64, 8, 32)
    w = np.array([1 / 3] + [1 / 18] * 6 + [1 / 36] * 12)[:, None, None, None]
    scale = np.ones((1, n[2], 1, 1))
    scale[:, 16:] = 2.0                              # slab 1: total density 3, slab 0: 1.5
    f0 = np.ascontiguousarray(np.broadcast_to(w * scale, (19, n[2], n[1], n[0])))
    g0 = 0.5 * f0
    ring = pkg.LocalSlabRing(*n, 2)
    ring.LBM_init(f0, g0)
    tm = [e.state_total_max for e in ring.engines]
    assert tm[0] == tm[1] and abs(tm[0] - 3.0) < 1e-12, tm
    ring.close()


def test_distributed_driver_world_size_one(pkg, ob):
    """SlabLattice over torch.distributed with one rank on the GPU (stream sharing with torch)."""
    import os
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        lat = pkg.SlabLattice(12, 12, 12, device=torch.device("cuda", 0))
        lat.LBM_init_droplet(0.3)
        lat.LBM_timestep(5)
        torch.cuda.synchronize()
        ref = ob.OracleLattice(12, 12, 12)
        ref.init_droplet(0.3)
        for _ in range(5):
            ref.timestep()
        f, g = lat.populations()
        _same(f, ref.f, "f")
        np.testing.assert_allclose(lat.update_com(), ref.com(), rtol=1e-12)
        np.testing.assert_allclose(lat.mass(), [ref.hbar[0].sum(), ref.hbar[1].sum()], rtol=1e-12)
        lat.close()
    finally:
        dist.destroy_process_group()


def _gloo_gpu_worker(rank, world, port, outdir, n, steps, par, staged=False, schedule=None):
    import os
    import sys
    if staged:
        os.environ["BFLBM_SLAB_STAGED"] = "1"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    lat = pkg.SlabLattice(*n, params=pkg.default_params(**par), device=torch.device("cuda", 0), schedule=schedule)
    assert lat.direct == (not staged)
    lat.LBM_init_droplet(0.3)
    lat.LBM_timestep(steps)
    torch.cuda.synchronize()
    f, g = lat.populations()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), f=f, g=g, h=lat.LBM_hydrovars(), z0=lat.z0, z1=lat.z1,
             com=lat.update_com(), mass=np.array(lat.mass()))
    # restart of a fluctuating run (main_run_job.cpp:80 step_continue, :253-270): a second lattice takes the populations through
    # LBM_init and the absolute step through set_steps_done, and continues the noise stream where the first one is
    again = pkg.SlabLattice(*n, params=pkg.default_params(**par), device=torch.device("cuda", 0), schedule=schedule)
    again.LBM_init(np.ascontiguousarray(f), np.ascontiguousarray(g))
    again.set_steps_done(steps)
    assert again.steps_done == steps == lat.steps_done
    lat.LBM_timestep(2); again.LBM_timestep(2)
    torch.cuda.synchronize()
    fc, gc = lat.populations()
    fr, gr = again.populations()
    np.savez(os.path.join(outdir, f"restart{rank}.npz"), fc=fc, gc=gc, fr=fr, gr=gr)
    dist.barrier()
    lat.close(); again.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,staged", [(2, False), (3, False), (2, True)], ids=["2-direct", "3-direct", "2-staged"])
def test_distributed_driver_ranks_sharing_one_gpu(ob, world, staged):
    """The real driver (slab.SlabLattice + HIP engine + torch.distributed P2P on device memory), `world` ranks on the
    one GPU of the test box over gloo (RCCL refuses several ranks per device).  Default transport: 38 plane-sized
    sends and receives per face between the state buffers themselves (bflbm_halo_planes, no staging kernels);
    BFLBM_SLAB_STAGED=1: pack -> one message per face -> unpack."""
    import socket
    import tempfile
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    n, steps, par = (10, 9, 16), 5, dict(kBT=1e-5, alpha0=2.0, seed=5)
    with tempfile.TemporaryDirectory() as d:
        mp.get_context("spawn")
        mp.spawn(_gloo_gpu_worker, args=(world, port, d, n, steps, par, staged), nprocs=world, join=True)
        ref = ob.OracleLattice(*n, params=ob.default_params(**par))
        ref.init_droplet(0.3)
        for _ in range(steps):
            ref.timestep()
        for r in range(world):
            o = np.load(os.path.join(d, f"r{r}.npz"))
            z0, z1 = int(o["z0"]), int(o["z1"])
            _same(o["f"], ref.f[:, z0:z1], f"rank {r} f")
            _same(o["g"], ref.g[:, z0:z1], f"rank {r} g")
            _same(o["h"], ref.h[:, z0:z1], f"rank {r} hydrovs")
            np.testing.assert_allclose(o["com"], ref.com(), rtol=1e-12)
            np.testing.assert_allclose(o["mass"], [ref.hbar[0].sum(), ref.hbar[1].sum()], rtol=1e-12)
        for _ in range(2):
            ref.timestep()
        for r in range(world):                              # the restarted lattice == the uninterrupted one == the oracle
            o, rs = np.load(os.path.join(d, f"r{r}.npz")), np.load(os.path.join(d, f"restart{r}.npz"))
            z0, z1 = int(o["z0"]), int(o["z1"])
            _same(rs["fr"], rs["fc"], f"rank {r} restarted f")
            _same(rs["gr"], rs["gc"], f"rank {r} restarted g")
            _same(rs["fc"], ref.f[:, z0:z1], f"rank {r} f after the continuation")


def test_distributed_driver_with_the_handover_schedule(ob):
    """Two ranks (one GPU, gloo), a lattice of full tiles, the hand-over kernel in every slab's interior sweep and
    boundary pairs, plane-sized sends between the state buffers: the oracle at tolerance."""
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import tolerances
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    n, steps, par = (128, 12, 24), 12, dict(alpha0=2.0)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_gloo_gpu_worker, args=(2, port, d, n, steps, par, False, "handover"), nprocs=2, join=True)
        ref = ob.OracleLattice(*n, params=ob.default_params(**par))
        ref.init_droplet(0.3)
        for _ in range(steps):
            ref.timestep()
        exact = True
        for r in range(2):
            o = np.load(os.path.join(d, f"r{r}.npz"))
            z0, z1 = int(o["z0"]), int(o["z1"])
            tolerances.check(o["h"], ref.h[:, z0:z1], f"rank {r}")
            assert np.abs(o["f"] - ref.f[:, z0:z1]).max() < 1e-13
            exact = exact and np.array_equal(o["f"], ref.f[:, z0:z1])
        assert not exact                                   # the frames were in use


def _bench(args, env=None, timeout=900):
    """`bench.py --gpus N` as the driver launches it (torch.distributed.run, one supervisor rank per GPU), rehearsed on the
    one GPU of this box: RCCL refuses several ranks per device, so the rccl transports run over gloo (BFLBM_BENCH_BACKEND)
    with the ranks sharing the device, and the peer transports put every slab on device 0.  A rehearsal of the code
    paths, never a measurement.  --full: the lines are checked for the repeated blocks and the exchange-after-sweep leg."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    n = args[args.index("--gpus") + 1]
    e = dict(os.environ, BFLBM_BENCH_BACKEND="gloo", **(env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", n, "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py")] + list(args) + ["--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=timeout, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout
    return json.loads(line[0]), out.stderr


def _check_line(r, transport_text):
    assert r["n_gpus"] == 2 and r["config"]["schedule"] == "handover" and r["scaling"] == "weak"
    assert r["config"]["workload"].startswith("128x16x24")
    assert r["config"]["halo_bytes_per_face"] == 38 * 128 * 16 * 8
    assert transport_text in r["config"]["halo_transport"], r["config"]["halo_transport"]
    rho, phi = r["config"]["mass_check"]
    assert abs(rho + phi - 128 * 16 * 24) < 1e-6            # rho + phi = rho_hi + rho_lo = 1 at every site of a stripe
    assert len(r["spread"]["blocks_ms_per_step"]) == 3 and r["value"] > 0
    ov = r["config"]["halo_overlap"]
    assert ov and ov["ms_per_step_exchange_after_sweep"] > 0


def test_bench_two_slabs_on_one_gpu_default_chain(tmp_path):
    """The N > 1 bench path with the hand-over schedule (what auto runs on the 512^3 slabs of the real bench) as the driver
    starts it: the first transport of the chain (rccl, staged) produces the line -- one JSON line with n_gpus 2, the stripe's
    mass conserved, the halo size and the transport stated, the exchange-after-sweep leg timed -- and the next transport
    family (the native ring with the copy engine, one process) is timed beside it as an informational leg (--second-transport).
    --dump-outputs: both transports write the sample of rank 0's slab (z < 12) and the lattice's mass."""
    d = str(tmp_path / "out")
    r, _ = _bench(["--gpus", "2", "--steps", "4", "--warmup", "2", "--shape", "128,16,12", "--schedule", "handover", "--second-transport",
                   "--dump-outputs", d])
    _check_line(r, "rccl, staged")
    f, g, h, mass = (np.load(os.path.join(d, k + ".npy")) for k in ("f", "g", "hydrovars", "mass"))
    assert f.shape == g.shape == (16, 19, 12, 16, 16) and h.shape == (16, 22, 12, 16, 16)
    assert np.isfinite(f).all() and np.isfinite(g).all() and np.isfinite(h).all()
    assert abs(mass.sum() - 128 * 16 * 24) < 1e-6
    tried = r["config"]["launcher"]["transports_tried"]
    assert [(t["transport"], t["ok"]) for t in tried] == [("rccl", True), ("peer-copy", True)]
    second = r["config"]["second_transport"]
    assert "copy engine" in second["halo_transport"] and "0 faces by kernel, 4 by copies" in second["halo_transport"]
    assert second["value"] > 0 and second["halo_overlap"]["ms_per_step_exchange_after_sweep"] > 0


def test_bench_falls_back_to_fresh_workers_with_the_next_transports():
    """rccl: the last rank dies before the rendezvous (what an RCCL abort looks like from outside); peer-copy: its one worker
    exits with an error.  The supervisors end what is left, start fresh workers with the next transport each time, the
    ring with in-place peer reads produces the line, and the remaining family member (rccl, direct: 38 plane-sized sends
    per face) is timed beside it -- so all four transports have run on this GPU between this test and the previous one."""
    r, err = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--shape", "128,16,12", "--schedule", "handover", "--second-transport"],
                    env={"BFLBM_BENCH_FAIL": "rccl:exit,peer-copy:exit"})
    _check_line(r, "a gather kernel reads")
    assert "4 faces by kernel, 0 by copies" in r["config"]["halo_transport"]
    tried = r["config"]["launcher"]["transports_tried"]
    assert [(t["transport"], t["ok"]) for t in tried] == [("rccl", False), ("peer-copy", False), ("peer-kernel", True), ("rccl-direct", True)]
    assert "rccl, direct" in r["config"]["second_transport"]["halo_transport"]
    assert err.count("FAILED") == 2


def test_bench_config3_slab_shape_two_ranks_sharing_the_gpu():
    """configs[3]'s slab shape as bench.py times it under config.also at N = 4: 512x512x128 per rank, droplet r = 0.2,
    `auto` (-> the hand-over kernel in the interior sweep, pulled rings in the boundary pairs); two ranks here."""
    r, _ = _bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--shape", "512,512,128", "--init", "droplet", "--transport", "rccl", "--blocks", "1", "--no-overlap-leg"],
                  env={"BFLBM_PLACEMENT_CANDIDATES": "2"})                 # with the placement tuning of bflbm_create on, in both ranks
    assert r["config"]["schedule"] == "handover" and r["config"]["slab_per_gpu"] == "512x512x128"
    assert r["config"]["placement"] and len(r["config"]["placement"]["candidates_ms_per_step"]) >= 1
    rho, phi = r["config"]["mass_check"]
    assert abs(rho + phi - 512 * 512 * 256) < 1e-3
    assert r["config"]["halo_bytes_per_face"] == 38 * 512 * 512 * 8


def test_ring_transports_and_overlap_switch(pkg, ob):
    """The native ring's faces by the gather kernel (default), by the copy engine (hipMemcpyPeerAsync per plane: the CU-free
    transport), and with the exchange after the sweep instead of behind it: the same doubles, and the ring says what moved."""
    n, par = (70, 9, 20), dict(kBT=1e-5, alpha0=2.0, seed=5)
    ref = ob.OracleLattice(*n, params=ob.default_params(**par))
    ref.init_droplet(0.3)
    for _ in range(6):
        ref.timestep()
    for transport, overlap, faces in (("kernel", True, (8, 0)), ("copy", True, (0, 8)), ("kernel", False, (8, 0)), ("copy", False, (0, 8))):
        ring = pkg.RingLBM(*n, nslabs=4, devices=(0,), params=pkg.default_params(**par), schedule="two_pass")
        ring.set_transport(transport)
        ring.set_overlap(overlap)
        ring.LBM_init_droplet(0.3)
        ring.LBM_timestep(6)
        assert ring.last_transport() == faces
        f, g = ring.populations()
        _same(f, ref.f, f"f {transport} overlap {overlap}")
        _same(g, ref.g, f"g {transport} overlap {overlap}")
        ring.close()


@pytest.mark.parametrize("schedule", ["two_pass", "fused"])
@pytest.mark.parametrize("nslabs,n", [(1, (8, 8, 8)), (2, (8, 8, 8)), (3, (10, 6, 13)), (4, (70, 9, 16))])
def test_native_ring(pkg, ob, nslabs, n, schedule):
    """bflbm_ring_*: the single-process ring inside the C-ABI (peer copies on a second stream overlapped
    with the interior planes), all slabs on the one GPU of the box, against the single-box oracle."""
    par = dict(kBT=1e-5, alpha0=2.0, seed=31)
    ring = pkg.RingLBM(*n, nslabs=nslabs, devices=(0,), params=pkg.default_params(**par), schedule=schedule)
    ref = ob.OracleLattice(*n, params=ob.default_params(**par))
    ring.LBM_init_droplet(0.3)
    ref.init_droplet(0.3)
    ring.LBM_timestep(7)
    for _ in range(7):
        ref.timestep()
    f, g = ring.populations()
    _same(f, ref.f, "f")
    _same(g, ref.g, "g")
    _same(ring.LBM_hydrovars(), ref.h, "hydrovs")
    _same(ring.thermal_noise()[0], ref.fn, "fnoise")
    np.testing.assert_allclose(ring.update_com(), ref.com(), rtol=1e-12)
    assert ring.steps_done == 7
    # restart from populations through the ring (upload faces exchanged natively)
    rng = np.random.default_rng(9)
    f0 = ref.f * (1 + 0.01 * rng.standard_normal(ref.f.shape))
    g0 = ref.g * (1 + 0.01 * rng.standard_normal(ref.g.shape))
    ring.LBM_init(f0, g0)
    ref.init_from(f0, g0)
    ring.LBM_timestep(3)
    for _ in range(3):
        ref.timestep()
    f, g = ring.populations()
    _same(f, ref.f, "f after ring LBM_init")
    _same(g, ref.g, "g after ring LBM_init")
    ring.close()


def test_native_ring_256_matches_single_context(pkg):
    """Overlap hazards show up at size: 4 slabs of 256x256x64 vs the single 256^3 context, 12 steps."""
    n = 256
    a = pkg.BinaryLBM(n, n, n, schedule="fused")
    a.LBM_init_droplet(0.2)
    a.LBM_timestep(12)
    ha = a.LBM_hydrovars_density()
    a.close()
    r = pkg.RingLBM(n, n, n, nslabs=4, devices=(0,), schedule="fused")
    r.LBM_init_droplet(0.2)
    r.LBM_timestep(12)
    hr = r.LBM_hydrovars_density()
    r.close()
    assert np.array_equal(ha, hr)


def test_native_ring_per_plane_copy_fallback():
    """the native ring has two transports -- k_halo_pull reading the neighbour's planes in place (peer
    mappings between GPUs) and 76 hipMemcpyPeerAsync per slab where no peer mapping exists.  On a one-GPU box the
    second never ran; BFLBM_RING_COPY_FALLBACK=1 forces it (fresh process: the switch is read once).  Both equal
    the oracle bit for bit; placement on more than one GPU stays unverified here."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import __graft_entry__ as ge, oracle_binding as ob\n"
            "pkg = ge.load_package()\n"
            "n = (70, 9, 16); par = dict(kBT=1e-5, alpha0=2.0)\n"
            "r = pkg.RingLBM(*n, nslabs=3, params=pkg.default_params(**par), schedule='two_pass')\n"
            "r.LBM_init_droplet(0.3); r.LBM_timestep(6); f, g = r.populations(); r.close()\n"
            "o = ob.OracleLattice(*n, params=ob.default_params(**par)); o.init_droplet(0.3)\n"
            "[o.timestep() for _ in range(6)]\n"
            "print('EQUAL', bool(np.array_equal(f, o.f) and np.array_equal(g, o.g)))\n") % (root, os.path.join(root, "tests"))
    for env in ({}, {"BFLBM_RING_COPY_FALLBACK": "1"}):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "EQUAL True" in out.stdout, (env, out.stdout[-500:], out.stderr[-1500:])


@pytest.mark.parametrize("n,nslabs", [((64, 8, 12), 3), ((128, 8, 16), 4), ((64, 8, 13), 3)])
def test_auto_on_slabs_that_are_all_boundary_planes(pkg, ob, n, nslabs):
    """A ring whose slabs are 4-5 planes thick has an EMPTY interior sweep; `auto` plans the kernels' chunking to pick
    a schedule and must not divide by that zero (it did, once: SIGFPE in round 3).  Default schedule, lattices wide
    enough for the hand-over kernel to be considered; 3 steps equal the oracle bit for bit (auto resolves to an exact
    schedule for such slabs)."""
    r = pkg.RingLBM(*n, nslabs=nslabs)
    r.LBM_init_droplet(0.45)
    r.LBM_timestep(3)
    f, g = r.populations()
    r.close()
    ref = ob.OracleLattice(*n)
    ref.init_droplet(0.45)
    for _ in range(3):
        ref.timestep()
    assert np.array_equal(f, ref.f) and np.array_equal(g, ref.g)
