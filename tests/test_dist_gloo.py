"""world_size-2 gloo tests (CPU) of the N>1 path: tenant partitioning / routing, mask sharding for tensor parallel
(N-split needs no exchange, K-split partial sums all-reduce to the full result) and the bench timing contract."""
import os
import socket
import sys

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from bitdelta_amd import dist as bdd
    from oracle import bd_oracle as o
    r, w, _ = bdd.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    torch.manual_seed(0)                                   # same problem on every rank
    M, K, N = 5, 128, 64
    x = torch.randn(1, M, K).bfloat16()
    p = torch.randint(-2 ** 31, 2 ** 31 - 1, (1, K // 32, N), dtype=torch.int64).to(torch.int32)
    full = o.delta_bmm(x, p, out_dtype=torch.float32, round_mode=0)
    # K-split (row-parallel): partial sums + all-reduce == full
    pk = bdd.shard_mask_rows(p, rank, world)
    xk = x[..., rank * (K // world):(rank + 1) * (K // world)].contiguous()
    part = o.delta_bmm(xk, pk, out_dtype=torch.float32, round_mode=0)
    tot = bdd.all_reduce_partial(part.clone())
    ok_k = torch.allclose(tot, full, rtol=1e-6, atol=1e-5)
    # N-split (column-parallel): slices concatenate to the full result, no exchange
    pn = bdd.shard_mask_columns(p, rank, world)
    coln = o.delta_bmm(x, pn, out_dtype=torch.float32, round_mode=0)
    gathered = [torch.empty_like(coln) for _ in range(world)]
    dist.all_gather(gathered, coln)
    ok_n = torch.equal(torch.cat(gathered, dim=-1), full)
    # tenant partition: disjoint cover, routing consistent
    mine = bdd.tenants_for_rank(7, rank, world)
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([len(mine)]))
    ok_t = sum(int(s) for s in sizes) == 7 and all(bdd.route(t, 7, world) == rank for t in mine)
    # timing contract: MAX over ranks
    import time
    dt = bdd.timed_region(lambda: time.sleep(0.02 * (rank + 1)), steps=2)
    ok_time = dt >= 0.02 * world * 2 * 0.95
    q.put((rank, ok_k, ok_n, ok_t, ok_time))
    dist.destroy_process_group()


def test_world_size_2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok_k, ok_n, ok_t, ok_time in res:
        assert ok_k and ok_n and ok_t and ok_time, (rank, ok_k, ok_n, ok_t, ok_time)


def test_partition_helpers_single_process():
    from bitdelta_amd import dist as bdd
    for n in (1, 6, 7, 32, 33):
        for world in (1, 2, 4, 8):
            cover = []
            for r in range(world):
                mine = bdd.tenants_for_rank(n, r, world)
                cover += mine
                assert all(bdd.route(t, n, world) == r for t in mine)
            assert cover == list(range(n))
    m = torch.arange(8 * 6, dtype=torch.int32).reshape(8, 6)
    assert torch.equal(torch.cat([bdd.shard_mask_rows(m, r, 4) for r in range(4)], 0), m)
    assert torch.equal(torch.cat([bdd.shard_mask_columns(m, r, 2) for r in range(2)], 1), m)


# ------------------------------------------------------------------------------------------------ PartialSumReducer: the transport decision is collective
def _reducer_worker(rank, world, port, q):
    """The one-shot (symmetric-memory) path of tp.PartialSumReducer may only be taken when EVERY rank could set it up: a rank that fell
    back to the ring while its peers sat in the rendezvous would hang the job.  Driven over gloo with the symmetric-memory
    primitives replaced by stand-ins, so that each failure mode can be injected on ONE rank: (a) nothing fails -> one-shot on all ranks;
    (b) enable fails on rank 1 -> ring on all ranks; (c) buffer allocation fails on rank 0 -> ring on all ranks for that shape, and the
    decision is cached; (d) the real class on a gloo group -> ring, no vote needed.  Every call must still return the correct sum."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from bitdelta_amd import dist as bdd
    from bitdelta_amd import tp
    bdd.init_from_env(backend="gloo")

    class Fake(tp.PartialSumReducer):
        fail_enable_on = fail_alloc_on = None
        rendezvous_calls = 0

        def _capable(self, device):
            return True

        def _local_enable(self):
            if self.fail_enable_on == dist.get_rank():
                raise RuntimeError("no peer access (injected)")
            self._gname = "fake"

        def _local_alloc(self, y):
            if self.fail_alloc_on == dist.get_rank():
                raise RuntimeError("symmetric allocation failed (injected)")
            return torch.empty(y.shape, dtype=y.dtype, device=y.device)      # y: (shape, dtype, device) of the message

        def _rendezvous(self, buf):
            self.rendezvous_calls += 1
            dist.barrier()                       # collective, like the real one: would hang if only some ranks got here

        def _one_shot(self, buf):
            out = buf.clone()
            dist.all_reduce(out)
            return out

    want = float(sum(range(1, world + 1)))
    res = {}
    y = lambda n=8: torch.full((2, n), float(rank + 1))
    a = Fake()
    out = a(y())
    res["all_ok"] = (bool((out == want).all()), a.calls["one_shot"], a.calls["ring"], a.report()["one_shot_available"])
    # producer-side use (RowParallelBinaryDiff): the Linear writes into the handed-out buffer, no staging copy; same cached buffer as above
    pbuf = a.buffer((2, 8), torch.float32, torch.device("cpu"))
    pbuf.fill_(float(rank + 1))
    res["producer_buffer"] = (pbuf is not None and bool((a.reduce_buffer(pbuf) == want).all()), a.calls["one_shot"], a.rendezvous_calls,
                              a.buffer((1024, 128), torch.float32, torch.device("cpu")) is None)
    b = Fake()
    b.fail_enable_on = 1
    out = b(y())
    res["enable_fails_on_rank1"] = (bool((out == want).all()), b.calls["one_shot"], b.calls["ring"], b.rendezvous_calls,
                                    b.report()["ring_reason"] is not None)
    c = Fake()
    c.fail_alloc_on = 0
    o1, o2, o3 = c(y()), c(y()), c(y(16))       # the failed shape stays on the ring (cached); another shape fails the same way
    res["alloc_fails_on_rank0"] = (bool((o1 == want).all() and (o2 == want).all() and (o3 == want).all()), c.calls["one_shot"], c.calls["ring"],
                                   c.rendezvous_calls)
    d = tp.PartialSumReducer()
    out = d(y())
    res["real_class_on_gloo"] = (bool((out == want).all()), d.calls["one_shot"], d.calls["ring"], "gloo" in (d.report()["ring_reason"] or ""))
    big = torch.full((1024, 128), float(rank + 1))                     # > ONE_SHOT_MAX_BYTES: ring whatever the setup says
    e = Fake()
    res["large_message"] = (bool((e(big) == want).all()), e.calls["one_shot"], e.calls["ring"])
    q.put((rank, res))
    dist.destroy_process_group()


def test_partial_sum_reducer_transport_decision_is_collective():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reducer_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, r in res:
        assert r["all_ok"] == (True, 1, 0, True), (rank, r)
        assert r["producer_buffer"] == (True, 2, 1, True), (rank, r)
        assert r["enable_fails_on_rank1"] == (True, 0, 1, 0, True), (rank, r)          # BOTH ranks on the ring, nobody in a rendezvous
        assert r["alloc_fails_on_rank0"] == (True, 0, 3, 0), (rank, r)
        assert r["real_class_on_gloo"] == (True, 0, 1, True), (rank, r)
        assert r["large_message"] == (True, 0, 1), (rank, r)


# ------------------------------------------------------------------------------------------------ tensor-parallel Linears through the HIP path
def _tp_worker(rank, world, port, q):
    """Two ranks share cuda:0 (the GPU box has one device); partial sums come from the HIP kernel (bd_binary_linear on the rank's
    K-slice / N-slice) and are reduced over gloo on host copies -- the same code path bench.py --workload tp70b drives over RCCL."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from bitdelta_amd import dist as bdd
    from bitdelta_amd import tp
    import bitdelta_amd as bd
    from oracle import bd_oracle as o
    bdd.init_from_env(backend="gloo")
    torch.manual_seed(0)                                   # same full problem on every rank
    res = {}
    for name, (N, K, M) in {"o_shard_like": (512, 256, 1), "down_like": (256, 1024, 3), "prefill": (384, 512, 200)}.items():
        base = (torch.randn(N, K) * 0.02).bfloat16()
        fine = (base.float() + torch.randn(N, K) * 5e-4).bfloat16()
        x = torch.randn(2, M, K).bfloat16()
        mask, coeff = o.binarize(base, fine)
        full = o.binary_linear(x.reshape(1, -1, K), base, mask[None], coeff.reshape(1, 1), out_dtype=torch.float32).reshape(2, M, N)
        dev = "cuda:0"
        # row parallel: K-slices, fp32 partials from the HIP kernel, all-reduce (gloo on host copies)
        rowp = tp.RowParallelBinaryDiff.from_full(base.to(dev), mask.to(dev), coeff.to(dev), rank, world)
        k = K // world
        part = rowp.partial(x[..., rank * k:(rank + 1) * k].contiguous().to(dev)).cpu()
        dist.all_reduce(part)
        ok_row = ((part - full).norm() / full.norm()).item() <= 1e-5
        # column parallel: N-slices concatenate to the full result, no exchange
        colp = tp.ColumnParallelBinaryDiff.from_full(base.to(dev), mask.to(dev), coeff.to(dev), rank, world)
        ycol = colp(x.to(dev)).float().cpu()
        gathered = [torch.empty_like(ycol) for _ in range(world)]
        dist.all_gather(gathered, ycol)
        ycat = torch.cat(gathered, dim=-1)
        ok_col = ((ycat - full).norm() / full.norm()).item() <= 4e-3 and ycat.shape == full.shape
        res[name] = (ok_row, ok_col)
    q.put((rank, res))
    dist.destroy_process_group()


import pytest  # noqa: E402


@pytest.mark.gpu
def test_tensor_parallel_linears_world_size_2_through_hip():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, res in out:
        for name, (ok_row, ok_col) in res.items():
            assert ok_row and ok_col, (rank, name, ok_row, ok_col)


# ------------------------------------------------------------------------------------------------ the TP decoder (fused shards, HIP glue)
TINY_TP = (1024, 2048, 2, 8, 2, 512)          # hidden, intermediate, layers, heads, kv heads, vocab: head_dim 128, 4 q heads per kv head


def _tp_decoder_worker(rank, world, port, q, backend):
    """Both ranks build the SAME full synthetic model and keep their shards; prefill + 3 decode steps (eager and via decode_runner) must
    give the logits of the world = 1 decoder built from the same full weights."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank if backend == "nccl" else 0), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from bitdelta_amd import dist as bdd
    from bitdelta_amd import tp
    if world > 1:
        bdd.init_from_env(backend=backend)
    dev = f"cuda:{rank}" if backend == "nccl" else "cuda:0"
    torch.cuda.set_device(dev)
    hid, inter, nl, heads, kvh, vocab = TINY_TP
    hd = hid // heads
    g = torch.Generator(device=dev).manual_seed(11)
    shapes = [(heads * hd, hid), (kvh * hd, hid), (kvh * hd, hid), (hid, heads * hd), (inter, hid), (inter, hid), (hid, inter)]
    full = [[tp.synth_full(o_, i_, dev, torch.float16, g) for o_, i_ in shapes] for _ in range(nl)]

    def run(r, w):
        dec = tp.TPDecoder(TINY_TP, dev, torch.float16, r, w, seed=3, full=full, max_len=256)
        ids = torch.randint(0, vocab, (1, 40), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        cache = dec.new_cache(128)
        outs = [dec(ids, torch.arange(40, device=dev), cache).float().cpu()]
        tok = torch.full((1, 1), 7, dtype=torch.long, device=dev)
        pos = torch.tensor([40], device=dev)
        runner, buf = dec.decode_runner(tok, pos, cache, use_graph=True)
        for _ in range(3):
            runner()
            torch.cuda.synchronize()
            outs.append(buf.float().cpu().clone())
        # a prefill CHUNK that starts at pos > 0 (must stay causal): same logits as the one-shot prefill of all 43 + 5 tokens
        return outs
    ref = run(0, 1) if rank == 0 else None
    got = run(rank, world)
    ok = True
    if rank == 0:
        for a, b in zip(got, ref):
            ok = ok and ((a - b).norm() / b.norm()).item() <= 5e-3
    q.put((rank, ok))
    if world > 1:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_tp_decoder_world_size_2_gloo_on_one_gpu():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_decoder_worker, args=(r, 2, port, q, "gloo")) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok for _, ok in out), out


@pytest.mark.gpu
def test_tp_decoder_world_size_2_rccl():
    """the same check over RCCL (one-shot symmetric-memory exchange for the decode messages, hipGraph replay of the per-rank step):
    needs two GPUs -- skipped on the one-GPU box, there for the day a multi-GPU node runs the suite"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_decoder_worker, args=(r, 2, port, q, "nccl")) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert all(ok for _, ok in out), out


@pytest.mark.gpu
def test_tp_decoder_chunked_prefill_is_causal():
    """world = 1: prefill in two chunks (the second starts at pos > 0) == prefill in one go (the old layer passed
    is_causal=False for such a chunk); and decode through the graph runner == eager decode"""
    sys.path.insert(0, ROOT)
    from bitdelta_amd import tp
    dev = "cuda:0"
    dec = tp.TPDecoder(TINY_TP, dev, torch.float16, 0, 1, seed=5, max_len=256)
    ids = torch.randint(0, 512, (1, 48), device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    c1 = dec.new_cache(128)
    one = dec(ids, torch.arange(48, device=dev), c1)
    c2 = dec.new_cache(128)
    dec(ids[:, :30], torch.arange(30, device=dev), c2)
    two = dec(ids[:, 30:], torch.arange(30, 48, device=dev), c2)
    assert ((one.float() - two.float()).norm() / one.float().norm()).item() <= 3e-3
    tok = torch.full((1, 1), 9, dtype=torch.long, device=dev)
    pos = torch.tensor([48], device=dev)
    eager = dec(tok, pos.clone(), c1).clone()
    pos2 = torch.tensor([48], device=dev)
    run, buf = dec.decode_runner(tok, pos2, c2, use_graph=True)
    run()
    torch.cuda.synchronize()
    assert ((eager.float() - buf.float()).norm() / eager.float().norm()).item() <= 3e-3 and int(pos2) == 49


# ------------------------------------------------------------------------------------------------ bench.py --gpus N launches N ranks itself
def _run_bench(argv, env_extra, timeout):
    import subprocess
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout,
                          env=env, cwd=ROOT)


def test_bench_gpus_n_reexecs_under_the_launcher_cpu():
    """`python bench.py --gpus 2` with no launcher in front (the driver's command line) must start TWO ranks under
    torch.distributed.run -- never silently measure one.  On this GPU-less box each rank then fails loudly (no CPU path): the failure
    report must come from the elastic launcher and name both the missing device and two local ranks."""
    r = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--layers", "1"], {"BD_DIST_BACKEND": "gloo"}, 300)
    if torch.cuda.is_available():
        import pytest
        pytest.skip("GPU box: covered by test_bench_gpus_2_runs_two_ranks_on_one_gpu")
    assert r.returncode != 0
    assert "needs a ROCm device" in r.stderr
    assert "torch.distributed" in r.stderr or "ChildFailedError" in r.stderr, r.stderr[-2000:]
    assert "local_rank: 1" in r.stderr or "rank      : 1" in r.stderr or "[rank1]" in r.stderr or "rank: 1" in r.stderr, r.stderr[-3000:]


def test_bench_world_size_mismatch_fails_loudly_cpu():
    """A launcher that started a different number of ranks than --gpus asks for is an error, not a one-rank measurement."""
    r = _run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "BD_DIST_BACKEND": "gloo",
                                                                   "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(_free_port())}, 120)
    assert r.returncode != 0


import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_gpus_2_runs_two_ranks_on_one_gpu():
    """bench.py --gpus 2 as the driver invokes it (no launcher): two ranks (gloo control plane, both on the box's one GPU), and the JSON
    line says so: n_gpus == n_ranks_seen == 2."""
    import json
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--layers", "1", "--full", "--no-mt-decode", "--no-cpu-baseline"],
                   {"BD_DIST_BACKEND": "gloo"}, 900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["n_ranks_seen"] == 2 and d["backend"] == "gloo"
    assert d["config"]["valid"] is False          # --layers 1 is a debug run and says so
    assert d["roofline"]["launches"] == 2 * 4 and d["roofline"]["ms_per_step_with_events"] > 0
