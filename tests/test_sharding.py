"""Multi-GPU layer: partition arithmetic, the optional gather over world_size-2 / -3 gloo groups on CPU (ranks shard the
REAL synthesiser output -- the HIP sources under the CPU emulator -- and the gathered batch must equal the unsharded one),
a sub-group that does not start at global rank 0, and on the MI355X a 1-rank RCCL communicator with G logical shards
(what a 1-GPU box can exercise of the G-GPU job)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_shard_bounds_cover_and_balance():
    from ddsp_svc_amd.sharding import shard_bounds, shard_counts
    for n in (0, 1, 7, 8, 512, 513):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            c = shard_counts(n, world)
            assert sum(c) == n and max(c) - min(c) <= 1
    with pytest.raises(ValueError):
        shard_bounds(4, 2, 2)


def _worker(rank, world, port, n_total, dst, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ddsp_svc_amd.sharding import gather_utterances, take_shard
    T = 6
    full = torch.arange(n_total * T, dtype=torch.float32).reshape(n_total, T)
    local = take_shard(full, rank, world) * 1.0          # each rank "synthesises" its own slice
    got = gather_utterances(local, n_total, dst=dst)
    ok = True
    if dst is None or rank == dst:
        ok = got is not None and torch.equal(got, full)
    else:
        ok = got is None
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.parametrize("n_total,dst", [(8, 0), (5, 0), (5, None), (1, 0)])
def test_gather_world2_gloo(n_total, dst):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + n_total * 7 + (0 if dst is None else 3)) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_total, dst, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok in res), res


def _worker_in_place(rank, world, port, n_total, dst, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if world > 1 or True:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from ddsp_svc_amd.sharding import gather_utterances, shard_bounds
    T = 6
    full = torch.arange(n_total * T, dtype=torch.float32).reshape(n_total, T)
    receiver = dst is None or rank == dst
    lo, hi = shard_bounds(n_total, rank, world)
    ok = True
    for step in range(2):                                   # the result tensor is kept from step to step
        if receiver:
            if step == 0:
                out = torch.full((n_total, T), -1.0)
            local = out[lo:hi]                              # the "synthesis" writes this rank's waveforms straight into its slice
            local.copy_(full[lo:hi] + step)
        else:
            out, local = None, full[lo:hi] + step
        got = gather_utterances(local, n_total, dst=dst, out=out)
        if receiver:
            ok = ok and got is out and torch.equal(got, full + step)
        else:
            ok = ok and got is None
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_total,dst", [(2, 8, 0), (2, 8, None), (1, 4, 0), (1, 4, None)])
def test_gather_into_the_callers_result_tensor_gloo(world, n_total, dst):
    """gather_utterances(out=): a receiving rank whose shard IS its slice of the result tensor (the synthesis wrote it there,
    synth.combsub_synth(signal_out=)) sends from there -- no copy of its own shard, nothing at all with one rank -- and the result is
    the caller's tensor, step after step"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() + world * 11 + n_total * 7 + (0 if dst is None else 3)) % 2000
    procs = [ctx.Process(target=_worker_in_place, args=(r, world, port, n_total, dst, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok in res), res


def _emu_backend():
    """what tests/backends.py's ``emu`` fixture does, for a spawned worker process"""
    import ctypes
    from ddsp_svc_amd import _ffi
    from tests.hipemu import build as emu_build
    _ffi._LIB = _ffi.bind(ctypes.CDLL(emu_build.build()))
    _ffi.check_device = lambda *t: None


def _synth_inputs(n_total, F, device):
    from oracle import ddsp_oracle as O
    f0 = torch.from_numpy(O.synth_f0(n_total, F, seed=77)).to(device)
    f0[0] = torch.clamp(f0[0] * 2.2, 65, 800)
    cg, ch, cn = (torch.from_numpy(c).to(device) for c in O.synth_controls(n_total, F, [33, 65, 17], seed=78))
    noise = torch.from_numpy(O.synth_noise(n_total, F * 512, seed=79)).to(device)
    return f0, cg, ch, cn, noise


def _combsub(f0, cg, ch, cn, noise):
    from ddsp_svc_amd import synth
    st = synth.phase(f0, 44100, 512)
    return synth.combsub_synth(f0, st, cg, ch, cn, noise, 44100, 512, want_components=False)[0]


def _synth_worker(rank, world, port, n_total, dst, use_async, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _emu_backend()
        from ddsp_svc_amd.sharding import gather_utterances, synth_sharded
        inputs = _synth_inputs(n_total, 5, "cpu")
        local = synth_sharded(_combsub, n_total, rank, world, *inputs)
        if use_async:
            finish, _ = gather_utterances(local, n_total, dst=dst, async_op=True)
            got = finish()
        else:
            got = gather_utterances(local, n_total, dst=dst)
        ok = True
        if dst is None or rank == dst:
            full = _combsub(*inputs)                                  # the unsharded batch, same kernels
            ok = got is not None and got.shape == full.shape and torch.equal(got, full) and bool(full.abs().max() > 1e-3)
        else:
            ok = got is None
        q.put((rank, ok))
    except Exception as e:                                            # surface the reason instead of a queue timeout
        q.put((rank, repr(e)))
    dist.destroy_process_group()


def _run(target, world, args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() * 7 + hash(args) % 997) % 2000
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    return res


@pytest.mark.parametrize("n_total,dst,use_async", [(4, 0, False), (3, 1, False), (3, None, True)])
def test_sharded_synth_world2_gloo(n_total, dst, use_async):
    """every rank synthesises its slice with the real kernels (emulated); gathered == unsharded, bit for bit"""
    res = _run(_synth_worker, 2, (n_total, dst, use_async))
    assert all(ok is True for _, ok in res), res


def _subgroup_worker(rank, world, port, n_total, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ddsp_svc_amd.sharding import gather_utterances, take_shard
        grp = dist.new_group([1, 2])                                  # does not contain global rank 0
        ok = True
        if rank in (1, 2):
            full = torch.arange(n_total * 4, dtype=torch.float32).reshape(n_total, 4)
            local = take_shard(full, rank - 1, 2)
            got = gather_utterances(local, n_total, dst=1, group=grp)  # group-local destination 1 = global rank 2
            ok = (got is not None and torch.equal(got, full)) if rank == 2 else got is None
        q.put((rank, ok))
    except Exception as e:
        q.put((rank, repr(e)))
    dist.destroy_process_group()


def test_gather_subgroup_world3_gloo():
    res = _run(_subgroup_worker, 3, (5,))
    assert all(ok is True for _, ok in res), res


@pytest.mark.gpu
def test_one_rank_rccl_logical_shards_gpu():
    """1-GPU box: a 1-rank RCCL communicator (backend nccl) + G = 4 logical shards of the real CombSub synthesis, gathered
    through the same call the 8-GPU job uses -> equal to the unsharded batch"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ddsp_svc_amd.sharding import gather_utterances, synth_sharded
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29700 + os.getpid() % 1000)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        probe = torch.ones(4, device=dev)
        dist.all_reduce(probe)                                         # the communicator works
        assert float(probe.sum()) == 4.0
        def same(a, b):          # the filter's workgroup run length may depend on the batch size: equal up to rounding
            return a.shape == b.shape and float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())
        inputs = _synth_inputs(8, 40, dev)
        full = _combsub(*inputs)
        local = synth_sharded(_combsub, 8, 0, 1, *inputs, logical_shards=4)
        for dst in (0, None):
            got = gather_utterances(local, 8, dst=dst)
            assert same(got, full)
        finish, _ = gather_utterances(local, 8, dst=0, async_op=True)
        assert same(finish(), full)
        # shard g of a G-GPU job == rows of the unsharded batch (what rank g of the 8-GPU run computes)
        for g in range(4):
            part = synth_sharded(_combsub, 8, g, 4, *inputs)
            assert same(part, full[2 * g:2 * g + 2])
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_a_live_rccl_communicator_does_not_slow_the_step_gpu():
    """Rounds 2 - 5: a process that had opened an RCCL communicator (every rank of a multi-GPU job) ran the B = 32 step ~10 % slower
    -- the communicator's streams pushed the synthesiser's SECOND stream onto the caller's hardware queue (EXPERIMENTS 5.3).  Round 6's
    default layout of a 256-bin step issues everything on the caller's stream (no second stream, no events): the step time with a
    live 1-rank communicator, default environment, stays within 5 % of the time without one (same process, same box)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import time
    from ddsp_svc_amd import synth
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    B, F = 32, 862
    from oracle import ddsp_oracle as O
    f0 = torch.from_numpy(O.synth_f0(B, F, seed=77)).to(dev)
    g = torch.Generator().manual_seed(5)
    cg, ch, cn = (torch.randn(B, F, 256, generator=g).to(dev) for _ in range(3))
    u = torch.rand(B, F * 512, generator=g).to(dev)

    def step():
        st = synth.phase(f0, 44100, 512)
        return synth.combsub_synth(f0, st, cg, ch, cn, u, 44100, 512, noise_is_u01=True, want_components=False)[0]

    def ms(reps=200):
        for _ in range(400):                                             # past the clocks' transient
            step()
        torch.cuda.synchronize()
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / reps * 1e3)
        return best
    before = ms()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29800 + os.getpid() % 1000)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        probe = torch.ones(4, device=dev)
        dist.all_reduce(probe)
        torch.cuda.synchronize()
        after = ms()
    finally:
        dist.destroy_process_group()
    assert after <= 1.05 * before, (before, after)
