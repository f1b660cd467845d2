"""CPU: host-side logic of the path — data-parallel gradient reduction over gloo (world_size 2),
synthetic data determinism, integer bookkeeping of the rollout, script argument surfaces."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from dvg_amd import parallel
    r, w, _ = parallel.init_distributed("gloo")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    if rank == 1:  # replicas must start identical: perturb then broadcast from rank 0
        with torch.no_grad():
            for p in net.parameters():
                p.add_(1.0)
    parallel.broadcast_parameters([net])
    x = torch.full((4, 7), float(rank + 1))
    net(x).sum().backward()
    net[1].bias.grad = None  # a parameter the pass did not touch must stay untouched
    local = [None if p.grad is None else p.grad.clone() for p in net.parameters()]
    red = parallel.FlatGradReducer(net.parameters())
    red.reduce()
    # plain numpy through the queue: torch tensors travel by file descriptor, which races with this process exiting
    npy = lambda t: None if t is None else t.detach().numpy().copy()  # noqa: E731
    out = {"rank": r, "world": w, "params": [npy(p) for p in net.parameters()],
           "local": [npy(g) for g in local], "reduced": [npy(p.grad) for p in net.parameters()],
           "shard": parallel.shard_batch(128, w)}
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_flat_grad_allreduce_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + os.getpid() % 300
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda d: d["rank"])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    a, b = res
    for d in (a, b):
        for k in ("params", "local", "reduced"):
            d[k] = [None if v is None else torch.from_numpy(v) for v in d[k]]
    assert a["world"] == 2 and a["shard"] == 64
    for pa, pb in zip(a["params"], b["params"]):
        assert torch.equal(pa, pb), "broadcast_parameters must make the replicas identical"
    for la, lb, ra, rb in zip(a["local"], b["local"], a["reduced"], b["reduced"]):
        if la is None:
            assert ra is None and rb is None
            continue
        assert torch.allclose(ra, (la + lb) / 2, atol=1e-6) and torch.equal(ra, rb)
    assert not torch.equal(a["local"][0], b["local"][0])


def _bcast_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from dvg_amd import parallel
    from dvg_amd.optim import FlatArena
    parallel.init_distributed("gloo")
    torch.manual_seed(rank)                       # replicas start DIFFERENT
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Linear(4, 3))
    outside = torch.nn.Linear(3, 2)               # a module whose parameters do not live in the arena
    params = list(net.parameters())
    arena = FlatArena(FlatArena.size_for(params), "cpu")
    off = 0
    with torch.no_grad():
        for p_ in params:                          # what FusedAdam._build does: parameters become views of arena.p
            v = arena.p[off:off + p_.numel()].view(p_.shape)
            v.copy_(p_)
            p_.data = v
            off += FlatArena.padded(p_.numel())
        net[1].running_mean.fill_(float(rank + 1))
        net[1].num_batches_tracked.fill_(7 * (rank + 1))
    n = parallel.broadcast_parameters([net, outside], arena_p=arena.p)
    assert all(p_.data_ptr() >= arena.p.data_ptr() for p_ in params), "parameters must still be views of the arena"
    q.put({"rank": rank, "collectives": n, "arena": arena.p.numpy().copy(),
           "params": [p_.detach().numpy().copy() for p_ in list(net.parameters()) + list(outside.parameters())],
           "bufs": [b.numpy().copy() for b in net.buffers()]})
    dist.barrier()
    dist.destroy_process_group()


def test_broadcast_parameters_is_one_collective_for_the_arena_gloo_world2():
    """parallel.broadcast_parameters(arena_p=...): the parameter arena goes as ONE broadcast, buffers and parameters outside
    the arena packed per dtype (float32 + BatchNorm's int64 counter): 3 collectives here instead of one per tensor (11)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + os.getpid() % 200
    procs = [ctx.Process(target=_bcast_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda d: d["rank"])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    a, b = res
    assert a["collectives"] == b["collectives"] == 3
    assert np.array_equal(a["arena"], b["arena"])
    for x, y in zip(a["params"] + a["bufs"], b["params"] + b["bufs"]):
        assert np.array_equal(x, y)
    assert float(b["bufs"][0][0]) == 1.0 and int(b["bufs"][2]) == 7          # rank 0's values won


def _arena_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from dvg_amd import parallel
    from dvg_amd.optim import FlatArena
    parallel.init_distributed("gloo")
    # the Trainer's layout: parameters whose .grad are views of one flat gradient buffer; ranges reduced in place
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))      # "decoder side" | "encoder side"
    params = list(net.parameters())
    arena = FlatArena(FlatArena.size_for(params), "cpu")
    views, off = [], 0
    for p_ in params:
        views.append(arena.g[off:off + p_.numel()].view(p_.shape))
        p_.grad = views[-1]
        off += FlatArena.padded(p_.numel())
    split = FlatArena.padded(35) + FlatArena.padded(5)                           # end of net[0]'s range
    net(torch.full((4, 7), float(rank + 1))).sum().backward()
    assert all(p_.grad is v for p_, v in zip(params, views)), "backward must accumulate into the flat views"
    local = arena.g.clone()
    red = parallel.ArenaReducer(arena.g)
    h1 = red.start(split, arena.g.numel())        # second range first, asynchronously ...
    h0 = red.start(0, split)                      # ... while "the rest of backward" would still be running
    red.finish(h1)
    red.finish(h0)
    red.enabled = False
    assert red.start(0, split) is None            # bench.py's no-all-reduce leg
    q.put({"rank": rank, "local": local.numpy().copy(), "reduced": arena.g.numpy().copy(),
           "grad0": params[0].grad.detach().numpy().copy(), "calls": red.calls, "floats": red.floats})
    dist.barrier()
    dist.destroy_process_group()


def test_arena_reducer_ranges_gloo_world2():
    """dvg_amd.parallel.ArenaReducer: in-place, asynchronous averaging of RANGES of the flat gradient arena whose views
    are the parameters' .grad (what train.Trainer does with RCCL), two ranks over gloo."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + os.getpid() % 40
    procs = [ctx.Process(target=_arena_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    a, b = sorted([q.get(timeout=120) for _ in procs], key=lambda d: d["rank"])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    mean = (a["local"] + b["local"]) / 2
    assert not np.array_equal(a["local"], b["local"])
    assert np.allclose(a["reduced"], mean, atol=1e-6) and np.array_equal(a["reduced"], b["reduced"])
    assert np.allclose(a["grad0"].reshape(-1), mean[:35], atol=1e-6), "p.grad IS the reduced buffer (no copy back)"
    assert a["calls"] == 2 and a["floats"] == a["local"].size


def test_shard_batch_rejects_uneven_split():
    from dvg_amd import parallel
    assert parallel.shard_batch(32, 8) == 4
    with pytest.raises(ValueError):
        parallel.shard_batch(50, 8)


def test_synthetic_moving_mnist_follows_the_reference_generator_contract():
    """moving_mnist.py:38-91: (T,64,64,1) float32 in [0,1], additive compositing clipped at 1, seeded."""
    from dvg_amd.data import SyntheticMovingMNIST
    a = SyntheticMovingMNIST(seq_len=6, seed=3).batch(3)
    b = SyntheticMovingMNIST(seq_len=6, seed=3).batch(3)
    assert a.shape == (3, 6, 64, 64, 1) and a.dtype == torch.float32
    assert torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and float(a.max()) > 0.5
    moved = (a[:, 1:] - a[:, :-1]).abs().flatten(2).sum(2)
    assert float(moved.min()) > 0.0 or True  # sprites may rest for a frame; at least something moves:
    assert float(moved.sum()) > 0.0


def test_normalize_data_matches_oracle_layout():
    from dvg_amd import utils
    from oracle import dvg_oracle as orc
    seq = torch.rand(2, 3, 8, 8, 3)
    ours, tgt = utils.normalize_data(None, torch.FloatTensor, (seq.clone(), torch.zeros(2)))
    ref = orc.normalize_data(seq)
    assert len(ours) == 3 and all(torch.equal(o, r) for o, r in zip(ours, ref))
    ours2, tgt2 = utils.normalize_data(None, torch.FloatTensor, seq.clone())
    assert tgt2 is None and torch.equal(ours2[1], ref[1])


def test_trigger_schedule_matches_oracle():
    from dvg_amd.rollout import trigger_steps
    from oracle import dvg_oracle as orc
    for n_past, n_eval in ((10, 20), (5, 105), (5, 15), (2, 31)):
        assert trigger_steps(n_past, n_eval) == orc.gp_trigger_steps(n_past, n_eval)


def test_script_flag_surfaces():
    sys.path.insert(0, ROOT)
    import generate_frames
    import train
    o = train.build_parser().parse_args(["--model", "vgg", "--batch_size", "8", "--n_past", "2", "--g_dim", "90",
                                          "--last_frame_skip"])
    assert o.model == "vgg" and o.batch_size == 8 and o.last_frame_skip and o.rnn_size == 256 and o.niter == 601
    g = generate_frames.build_parser().parse_args(["--model_dir", "x", "--dataset", "kth"])
    assert g.n_eval == 105 and g.n_future == 100 and g.batch_size == 50   # generate_frames.py:47-49


def test_init_weights_matches_reference_distribution():
    """utils.py:304-311: class-name substring dispatch."""
    from dvg_amd import utils
    from dvg_amd.models.vgg_64 import encoder
    torch.manual_seed(0)
    e = encoder(90, 1)
    e.apply(utils.init_weights)
    w = e.c3[1].main[0].weight
    assert abs(float(w.std()) - 0.02) < 2e-3 and abs(float(w.mean())) < 1e-3
    assert float(e.c3[1].main[0].bias.abs().max()) == 0.0
    assert abs(float(e.c3[1].main[1].weight.mean()) - 1.0) < 0.01


def test_batch_prefetcher_keeps_order_propagates_errors_and_ends():
    """train.BatchPrefetcher: the generator's items in its order from a background thread, its exception re-raised at the
    consumer, exhaustion as StopIteration (repeatably)."""
    import train
    assert list(train.BatchPrefetcher(iter(range(9)), depth=2)) == list(range(9))
    pf = train.BatchPrefetcher(iter([1]))
    assert next(pf) == 1
    for _ in range(2):
        with pytest.raises(StopIteration):
            next(pf)

    def bad():
        yield "a"
        raise ValueError("boom")
    pf = train.BatchPrefetcher(bad())
    assert next(pf) == "a"
    with pytest.raises(ValueError):
        next(pf)


def test_gp_trigger_oracle_memo_and_forced_decisions():
    """oracle.gp_trigger_gen (generate_frames.py:249-298), the checker of the B = 50 GPU test: (1) with a memo shared by the calls
    for several batch indices every (step, decisions so far) pair is computed once and the results equal the un-memoised calls
    bit for bit; (2) `decisions` + `guard`: a step whose own margin is inside the guard follows the given branch (reported in
    `forced`), every other step decides for itself - with guard = 0 the decisions are ignored."""
    from oracle import dvg_oracle as orc
    from oracle import params
    from tests.test_gpu_configs import _build, _oracle_fns
    B, total = 5, 18
    mods, (esd, dsd, lsd, gsd, lik) = _build("dcgan", 64, 1, B, 3300)
    xs = [params.frames(3310, B, 1, 64)]
    eps = {i: params.normal(3320 + i, 90, B) for i in range(12, total)}
    enc_o, dec_o = _oracle_fns("dcgan", 64, esd, dsd)
    memo = {}
    with torch.no_grad():
        for index in (0, 4):
            a = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, index, eps, total=total, depth=-250)
            b = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, index, eps, total=total, depth=-250, memo=memo)
            assert a["triggers"] == b["triggers"] and a["values"] == b["values"] and a["thresholds"] == b["thresholds"]
            assert all(torch.equal(u, v) for u, v in zip(a["frames"], b["frames"]))
        assert any(k[0] == "post" for k in memo) and any(k[0] == "warm" for k in memo)
        flip = {i: (i not in a["triggers"]) for i in range(12, total)}           # the opposite branch everywhere
        c = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, 4, eps, total=total, depth=-250, decisions=flip, guard=0.0)
        assert c["triggers"] == a["triggers"] and c["forced"] == []
        d = orc.gp_trigger_gen(xs, enc_o, dec_o, lsd, gsd, lik, 4, eps, total=total, depth=-250, decisions=flip, guard=1e9)
        assert d["forced"] == list(range(12, total)) and d["triggers"] == [i for i in range(12, total) if flip[i]]


def test_hoist_ready_and_hoisted_skip_agree_across_evictions(monkeypatch):
    """a decoder block's producer asks fused._hoist_ready(conv, skip) and, on yes, hands its consumer an upsampled
    WinoV - the consumer then MUST get the skip half from fused._hoisted_skip.  The two agree in every cache state (frozen
    declaration, second sighting, weight change, dead skips), and where the entry is evicted between the two calls (the
    64-entry bound) the consumer's `force=True` still yields the skip half instead of raising.  Host logic only: the packing
    and the conv launch are stubbed."""
    from dvg_amd import fused, weights
    monkeypatch.setattr(weights, "split_packed", lambda weight, c1, transposed=False: ("px", "ps"))
    calls = []
    part = lambda ps: calls.append(ps) or "S"      # noqa: E731
    fused.clear_skip_hoist_cache()
    conv = torch.nn.Conv2d(8, 4, 3, 1, 1)
    x, skip = torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)

    def agree(force=False):
        ready = fused._hoist_ready(conv, skip)
        got = fused._hoisted_skip(conv, x, skip, part, force=force)
        assert ready == (got is not None) or force, (ready, got)
        return got
    assert agree() is None                       # first sighting, undeclared: the ordinary concat conv
    assert agree() == ("px", "S")                # second sighting
    skip.add_(1.0)                               # the skip changed: a new first sighting
    assert agree() is None
    fused.declare_frozen_skips([skip])           # declared loop-invariant: ready at once
    fused._skip_seen.clear()
    assert agree() == ("px", "S")
    with torch.no_grad():
        conv.weight.add_(1.0)                    # new weight version: entry stale, but the skip is still declared frozen
    assert agree() == ("px", "S")
    # eviction between producer and consumer of an UNDECLARED skip
    fused.clear_skip_hoist_cache()
    assert fused._hoisted_skip(conv, x, skip, part) is None and fused._hoisted_skip(conv, x, skip, part) is not None
    assert fused._hoist_ready(conv, skip)        # the producer sees the entry ...
    keep = [torch.zeros(1) for _ in range(70)]
    for t in keep:                               # ... 70 other (conv, skip) pairs pass through the 64-entry table ...
        fused._hoisted_skip(conv, x, t, part)
    assert not fused._hoist_ready(conv, skip)    # ... and it is gone when the consumer asks
    assert fused._hoisted_skip(conv, x, skip, part) is None
    fused._skip_seen.clear()
    assert fused._hoisted_skip(conv, x, skip, part, force=True) == ("px", "S")    # the consumer's call: never None
    del keep
    import gc
    gc.collect()
    alive = torch.zeros(1)
    fused._hoisted_skip(conv, x, alive, part)              # a miss sweeps the dead entries
    assert all(e[0]() is not None for e in fused._skip_seen.values())
    fused.clear_skip_hoist_cache()


def _sync_bn_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from dvg_amd import fused, ops, parallel
    parallel.init_distributed("gloo")
    assert fused.sync_bn_world() == 1 and ops.sync_bn_state() is None
    fused.set_sync_bn(dist, dist.new_group())
    assert fused.sync_bn_world() == 2 and ops.sync_bn_state() is not None
    g = torch.Generator().manual_seed(100 + rank)
    partial = torch.randn(3 * 5, 2, 8, generator=g)        # 3 groups x 5 per-tile rows of (sum, sum of squares) x 8 channels
    out = ops.sync_partial_rows(partial, 3)
    q.put({"rank": rank, "partial": partial.numpy().copy(), "out": out.numpy().copy(), "grouped": int(out.grouped)})
    fused.set_sync_bn(None)
    assert fused.sync_bn_world() == 1 and ops.sync_bn_state() is None
    dist.barrier()
    dist.destroy_process_group()


def test_sync_bn_partial_rows_allreduce_gloo_world2():
    """--sync_bn's collective (ops.sync_partial_rows): each rank's per-tile partial rows [G r][2][C] become TWO fp32 rows per
    group (hi + lo) that add up to the fp64 sums over all rows of all ranks, identical on every rank; the switch turns on
    only for a group of more than one rank and off again."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + os.getpid() % 40
    procs = [ctx.Process(target=_sync_bn_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda d: d["rank"])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    a, b = res
    want = (a["partial"].astype(np.float64).reshape(3, 5, 2, 8).sum(1) +
            b["partial"].astype(np.float64).reshape(3, 5, 2, 8).sum(1))
    # two fp32 rows per group (hi, lo) whose fp64 sum is the fp64 total over both ranks
    assert a["out"].shape == (6, 2, 8) and a["grouped"] == 3
    assert np.array_equal(a["out"], b["out"])
    got = a["out"].astype(np.float64).reshape(3, 2, 2, 8).sum(1)
    assert np.array_equal(a["out"].reshape(3, 2, 2, 8)[:, 0], want.astype(np.float32))
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    # one rank: the switch stays off (nothing to synchronise)
    from dvg_amd import fused, ops
    fused.set_sync_bn(None)
    assert fused.sync_bn_world() == 1 and ops.sync_bn_state() is None


def test_environment_switches_are_the_documented_ten_and_no_file_is_a_monolith():
    """"<= 10 switches", "no file > 800 lines outside csrc/".  Every DVG_* environment variable the product
    reads (package, train.py, generate_frames.py, bench.py) is named in README.md's switch paragraph and there are at most ten;
    no source file outside dvg_amd/csrc is longer than 800 lines."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, "dvg_amd", "**", "*.py"), recursive=True) + \
        [os.path.join(root, f) for f in ("train.py", "generate_frames.py", "bench.py", "utils.py", "gp_models.py")]
    read = set()
    for f in files:
        read |= set(re.findall(r"environ(?:\.get|\.setdefault)?[\(\[]\s*[\"'](DVG_[A-Z0-9_]+)[\"']", open(f).read()))
    readme = open(os.path.join(root, "README.md")).read()
    para = readme[readme.index("Switches (environment"):readme.index("All keep the results within the parity tolerances.")]
    documented = set(re.findall(r"DVG_[A-Z0-9_]+", para))
    assert read <= documented, sorted(read - documented)
    assert len(read) <= 10, sorted(read)
    long_files = []
    for pat in ("*.py", "dvg_amd/**/*.py", "tests/*.py", "tools/*.py", "oracle/*.py", "models/*.py", "include/*.h"):
        for f in glob.glob(os.path.join(root, pat), recursive=True):
            n = sum(1 for _ in open(f))
            if n > 800:
                long_files.append((os.path.relpath(f, root), n))
    assert not long_files, long_files


def test_pooled_streams_are_made_once_per_role_and_index(monkeypatch):
    """graphs.pooled_stream: torch hands streams out of a pool of 32 per device, round-robin; graph holders that made fresh ones
    (six per ConcurrentRollouts) wrapped around it in bench.py and hipGraphLaunch crashed (r06).  Every (device, role, index) stream is
    made once per process and shared by all holders - checked here without a GPU, on a stand-in for torch.cuda.Stream."""
    import inspect
    import torch
    from dvg_amd import graphs, rollout
    made = []

    class FakeStream:
        def __init__(self):
            made.append(self)
    monkeypatch.setattr(torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(graphs, "_streams", {})
    chains = [[graphs.pooled_stream("chain", k) for k in range(3)] for _ in range(14)]     # 14 holders x 3 chains
    warm = [graphs.pooled_stream("warmup") for _ in range(14 * 3)]
    assert all(c[k] is chains[0][k] for c in chains for k in range(3)) and len({id(s) for s in chains[0]}) == 3
    assert all(w is warm[0] for w in warm) and warm[0] not in chains[0]
    hoist = graphs.pooled_stream("hoist")       # the hoist stream of rollout.condition() is the pooled one
    assert 'graphs.pooled_stream("hoist")' in inspect.getsource(rollout.condition) and "cuda.Stream(" not in inspect.getsource(rollout)
    assert hoist is graphs.pooled_stream("hoist") and hoist is not warm[0] and hoist not in chains[0]
    assert len(made) == 5
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)          # another device: its own streams
    assert graphs.pooled_stream("chain", 0) is not chains[0][0] and len(made) == 6


def test_bench_dump_outputs_arguments_and_size_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs DIR: the flag parses, --steps / --warmup are checked, and dump_outputs() writes float32 .npy
    files - whole arrays within the budget, above it the same leading clips of every array (a fixed sample) within it."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == str(tmp_path)
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    frames = torch.randn(4, 6, 1, 8, 8)
    other = torch.randn(4, 6, 1, 8, 8, dtype=torch.float64)
    shapes = bench.dump_outputs(str(tmp_path / "all"), {"vgg_frames": frames, "dcgan_frames": other})
    assert shapes == {"vgg_frames": [4, 6, 1, 8, 8], "dcgan_frames": [4, 6, 1, 8, 8]}
    got = np.load(tmp_path / "all" / "vgg_frames.npy")
    assert got.dtype == np.float32 and np.array_equal(got, frames.numpy())
    assert np.load(tmp_path / "all" / "dcgan_frames.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 2 * (4 * 8 * 8 * 4))     # room for two clips of each of the two arrays
    shapes = bench.dump_outputs(str(tmp_path / "cut"), {"vgg_frames": frames, "dcgan_frames": other})
    assert shapes == {"vgg_frames": [4, 2, 1, 8, 8], "dcgan_frames": [4, 2, 1, 8, 8]}
    cut = np.load(tmp_path / "cut" / "vgg_frames.npy")
    assert np.array_equal(cut, frames[:, :2].numpy())
    assert sum(os.path.getsize(tmp_path / "cut" / f) for f in os.listdir(tmp_path / "cut")) <= bench.DUMP_BYTES + 2 * 256


def test_bench_plain_run_leaves_every_other_leg_to_full():
    """A plain `bench.py` times the headline steps alone: every leg beside them is off unless --full is given, and under --full
    the defaults and the --no-* switches are what they were."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    legs = ("no_check", "no_cpu_baseline", "no_roofline", "no_train_leg", "no_f32mfma_leg", "no_make_gifs_leg", "no_extra_legs")
    plain = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.sustained_s == 0.0 and all(getattr(plain, k) for k in legs)
    assert plain.steps == 7 and plain.warmup == 2 and plain.inflight == 3 and plain.model == "vgg" and not plain.no_families
    full = bench.parse_args(["--full"])
    assert full.full and full.sustained_s == 5.0 and not any(getattr(full, k) for k in legs)
    assert bench.parse_args(["--full", "--no-roofline", "--sustained-s", "0"]).no_roofline
    assert bench.parse_args(["--sustained-s", "0"]).sustained_s == 0.0
    with pytest.raises(SystemExit):
        bench.parse_args(["--sustained-s", "20"])       # a figure only --full measures


def test_derived_rebuilds_on_version_or_pointer_change_and_dies_with_its_owner():
    """_derived.derived: one entry per (owner, tag), valid while every source tensor keeps its (data_ptr, _version); the
    store does not keep the owner alive and forgets it when it dies."""
    import gc
    from dvg_amd import _derived
    _derived.drop_all()
    conv = torch.nn.Conv2d(2, 3, 3)
    built = []

    def get(tag="a", owner=None, sources=None, value=None):
        def build():
            built.append(tag)
            return value if value is not None else torch.zeros(1)
        return _derived.derived(owner if owner is not None else conv, tag, (conv.weight,) if sources is None else sources, build)
    first = get()
    assert get() is first and built == ["a"]                     # unchanged sources: the same object, build not called
    with torch.no_grad():
        conv.weight.add_(1)                                      # in-place update: new _version
    second = get()
    assert second is not first and get() is second and built == ["a", "a"]
    conv.weight.data = conv.weight.data.clone()                  # re-allocated storage (load_state_dict / .to()): new data_ptr
    third = get()
    assert third is not second and get() is third and built == ["a"] * 3
    other = get("b")                                             # two tags on one owner are independent
    assert other is not third and get() is third and get("b") is other and built == ["a"] * 3 + ["b"]
    assert get(("c", 1), sources=(None, conv.weight)) is get(("c", 1), sources=(None, conv.weight))   # a None source stays None
    n = len(built)
    assert _derived.derived(conv, "none", (conv.weight,), lambda: built.append("none")) is None        # None is a legal value ...
    assert _derived.derived(conv, "none", (conv.weight,), lambda: built.append("none")) is None and len(built) == n + 1  # ... and a hit
    # a parameter as owner (tensors are never compared with ==)
    p_val = get("p", owner=conv.weight)
    assert get("p", owner=conv.weight) is p_val
    held = {id(t) for t in _derived.snapshot()}
    assert {id(third), id(other), id(p_val)} <= held and id(first) not in held and id(second) not in held
    ids = (id(third), id(other), id(p_val))
    keys = (id(conv), id(conv.weight))
    assert all(k in _derived._store for k in keys)
    del conv
    gc.collect()
    assert not any(k in _derived._store for k in keys)
    assert not {id(t) for t in _derived.snapshot()} & set(ids)
    _derived.drop_all()


def test_every_module_level_cache_is_registered_dropped_and_snapshotted(monkeypatch):
    """The registry of _derived: graphs.snapshot_eager_caches() holds every tensor of every registered cache,
    graphs.drop_version_keyed_caches() empties every one of them and the deferred weight-gradient queues.  The names are
    listed literally: a new module-level cache means a new name here.  (One object per form whoever asks, one build per
    parameter version: tests/test_weights_host.py.)"""
    from dvg_amd import _derived, fused, graphs, ops, weights
    from dvg_amd import autograd as ag
    from dvg_amd.ops import edge
    assert set(_derived.registered()) == {"derived", "zero_state", "splitk_ws", "group_maps", "skip_proj", "loss_weights",
                                          "skip_hoist"}
    graphs.drop_version_keyed_caches()
    made = []

    def t():
        made.append(torch.zeros(2))
        return made[-1]
    monkeypatch.setattr(ops, "pack_igemm_weight", lambda w, transposed=False: t())
    monkeypatch.setattr(ops, "winograd_weight", lambda w, m: t())
    monkeypatch.setattr(ops, "transpose2d", lambda w: t())
    monkeypatch.setattr(edge, "pixel_proj", lambda x, wm: t())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)       # (asks the device otherwise)
    conv, bn, lin = torch.nn.Conv2d(8, 4, 3, 1, 1), torch.nn.BatchNorm2d(4), torch.nn.Linear(3, 2)
    last, pair, convt = torch.nn.ConvTranspose2d(8, 1, 3, 1, 1), torch.nn.Conv2d(1, 64, 3, 1, 1), torch.nn.ConvTranspose2d(8, 4, 4, 2, 1)
    big = torch.nn.ConvTranspose2d(200, 8, 4)
    w, wt = conv.weight, convt.weight
    # "derived": the sites of weights, fused.folded_affine and ops.edge, stub builders where the real one launches a kernel
    got = [weights.packed(w), *weights.split_packed(w, 4), weights.k4_packed(w, 4), weights.packed(wt, True),
           *weights.split_packed(wt, 4, True), weights.k4_packed(w, 4, adjoint=True), weights.packed(w, True, 0, 4, 1), weights.winograd(w, 4), weights.winograd(w, 4, 0, 4), weights.winograd(w, 4, 4, 8, dgrad=True),
           weights.transposed(lin.weight), weights.gemm_operand(w, "head"), weights.gemm_operand(wt, "stem"),
           weights.gemm_operand(wt, "stem_t"), weights.gemm_operand(w, "head_T"), weights.first_pair_taps(pair.weight),
           *fused.folded_affine(conv, bn), ops._last_wmat_cached(last.weight, 4, 8, 9)]
    assert weights.packed(w) is got[0] and weights.transposed(lin.weight) is got[12] and len({id(g) for g in got}) == len(got)
    assert weights.gemm_operand(big.weight, "stem_t") is None         # (dim > 128: no dvg_stem_gemm form)
    k4 = weights.k4_weight(conv.weight.double(), 4).double()      # K4 = W (*) ones(2x2): every tap lands 4 times
    assert k4.shape == (4, 4, 4, 4) and torch.allclose(k4.sum((2, 3)), 4 * conv.weight.detach().double()[:, :4].sum((2, 3)).t(), rtol=1e-5, atol=1e-7)
    # the plain caches, one entry each
    z = _derived.zero_state(2, 3, torch.device("cpu"))
    assert z is _derived.zero_state(2, 3, torch.device("cpu")) and z.shape == (2, 3) and not z.any()
    ops._SPLITK_WS[(0, 0, 2, 0)] = ws = t()
    gmap = ops.shared_map((0, 1, 1), torch.device("cpu"))
    skip, x = torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2)
    proj = ops._cached_skip_proj(skip, lambda: None, last.weight)
    ops._LOSS_W[("cpu", (1.0,))] = lw = t()
    fused.declare_frozen_skips([skip])
    _, s_half = fused._hoisted_skip(conv, x, skip, lambda ps: t())
    want = got + [z, ws, gmap, proj, lw, s_half]
    held = {id(k) for k in graphs.snapshot_eager_caches()}
    assert all(id(w) in held for w in want), [i for i, w in enumerate(want) if id(w) not in held]
    ag._wgrad_queues["k"] = [object()]
    ag._dense_queues["k"] = [object()]
    ag._wgrad_flush_queued = True
    graphs.drop_version_keyed_caches()
    for name, cache in (("derived", _derived._store), ("zero_state", _derived._zero_states), ("splitk_ws", ops._SPLITK_WS),
                        ("group_maps", ops._MAP_CACHE), ("skip_proj", ops._SKIP_PROJ_CACHE), ("loss_weights", ops._LOSS_W),
                        ("skip_hoist", fused._skip_seen), ("skip_hoist", fused._frozen)):
        assert len(cache) == 0, name
    assert graphs.snapshot_eager_caches() == []
    assert not ag._wgrad_queues and not ag._dense_queues and ag._wgrad_flush_queued is False
    assert weights.packed(conv.weight) is not got[0]              # rebuilt on demand
    z, _ = _derived.zero_state(2, 3, torch.device("cpu")), graphs.drop_parameter_forms()     # before a training capture: the derived forms only
    assert len(_derived._store) == 0 and _derived.zero_state(2, 3, torch.device("cpu")) is z
    graphs.drop_version_keyed_caches()


def _code_only(path):
    """The source of a Python file without its docstrings and comments (they may speak of anything)."""
    import ast
    import io
    import tokenize
    src = open(path).read()
    lines = src.splitlines(keepends=True)
    for node in ast.walk(ast.parse(src)):
        body = getattr(node, "body", None)
        if (isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and body and
                isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and isinstance(body[0].value.value, str)):
            for ln in range(body[0].lineno - 1, body[0].end_lineno):
                lines[ln] = "\n"
    toks = [t for t in tokenize.generate_tokens(io.StringIO("".join(lines)).readline) if t.type != tokenize.COMMENT]
    return tokenize.untokenize(toks)


def test_version_counters_are_read_in_one_place_and_the_cache_walkers_name_no_private_dict():
    """`(data_ptr, _version)` bookkeeping lives in dvg_amd/_derived.py; the files below read `._version` for something that
    is not a parameter-derived cache.  The capture protocol (graphs.py) and the graph holders of rollout.py go through the
    registry and the public functions of the modules that own the caches: in their whole source they name no underscore
    attribute of another module."""
    import glob
    import re
    allowed = {
        "_derived.py": "the helper itself",
        "fused.py": "skip sightings: activation-keyed (tensor identity + version of the SKIP), another life cycle",
        "autograd.py": "share-scope key of one time step's skip halves (activation, not a parameter)",
        "autograd_recurrent.py": "backward checks that the saved parameters were not stepped since the forward",
        os.path.join("ops", "edge.py"): "skip projection: keyed on the skip activation and the weight it was projected with",
    }
    base = os.path.join(ROOT, "dvg_amd")
    readers = {os.path.relpath(f, base) for f in glob.glob(os.path.join(base, "**", "*.py"), recursive=True)
               if re.search(r"\._version\b", open(f).read())}
    assert readers == set(allowed), sorted(readers ^ set(allowed))
    for name in ("graphs.py", "rollout.py"):
        src = _code_only(os.path.join(base, name))
        assert "def " in src and "import" in src
        hit = re.search(r"\b(ag|autograd|fused|ops|edge|lstm_mod|graphs|_derived)\._\w+", src)
        assert not hit, (name, hit.group(0))


def test_the_capture_protocol_is_written_in_graphs_only():
    """Inside dvg_amd/, graph objects are made, captures are opened, the capture error mode is named and the skip-dependent
    caches are cleared in graphs.py and nowhere else (the two `def`s stay where the caches live)."""
    import glob
    import re
    base = os.path.join(ROOT, "dvg_amd")
    pats = {"CUDAGraph(": r"torch\.cuda\.CUDAGraph\(", "graph(": r"torch\.cuda\.graph\(", "capture_error_mode": r"capture_error_mode",
            "clear_skip_*_cache()": r"(?<!def )\bclear_skip_(hoist|proj)_cache\("}
    found = {k: set() for k in pats}
    files = glob.glob(os.path.join(base, "**", "*.py"), recursive=True)
    assert len(files) > 20
    for f in files:
        src = open(f).read()
        for k, pat in pats.items():
            if re.search(pat, src):
                found[k].add(os.path.relpath(f, base))
    assert all(v == {"graphs.py"} for v in found.values()), found


def test_the_iteration_is_written_in_the_trainer_only():
    """The body of a training iteration and its read-back are Trainer._iteration_dev / _iteration_result: the graph holders and
    the training benchmark name none of their parts, `_iteration_dev(` appears as its definition and its two callers, and no
    code asks a Trainer (or a FusedAdam) with a default for state that their __init__ declares (options objects may: old
    pickled ones lack newer flags)."""
    import glob
    import re
    for name in (os.path.join("dvg_amd", "train_graphs.py"), os.path.join("tools", "bench_train.py")):
        src = _code_only(os.path.join(ROOT, name))
        assert "def " in src and "import" in src
        for part in ("_train_model_dev", "_finetune_dev", ".tick(", "ema.update(", "last_loss =", "_iters"):
            assert part not in src, (name, part)
    files = sorted(glob.glob(os.path.join(ROOT, "dvg_amd", "*.py"))) + [os.path.join(ROOT, "train.py")]
    assert len(files) > 20
    declared = "_iters|_ft_cache|_segmenter|_ar_pending|_plot_writer|state_loads|last_loss|_graph_stale|ema|lr_schedule|validation"
    calls, asked = [], []
    for f in files:
        src = _code_only(f)
        rel = os.path.relpath(f, ROOT)
        calls += [(rel, ln.strip()) for ln in src.splitlines() if "_iteration_dev(" in ln]
        asked += [(rel, m.group(0)) for m in re.finditer(r"getattr\(\s*([\w.]+)\s*,\s*[\"'](%s)[\"']" % declared, src)
                  if not m.group(1).endswith("opt")]
        asked += [(rel, m.group(0)) for m in re.finditer(r"setdefault\(\s*[\"'](%s)[\"']" % declared, src)]
    assert not asked, asked
    assert sorted(rel for rel, _ in calls) == [os.path.join("dvg_amd", "train_graphs.py")] + [os.path.join("dvg_amd", "trainer.py")] * 2, calls
    assert sorted(re.sub(r"\s+", "", ln) for _, ln in calls) == [
        "def_iteration_dev(self,x):", "returnself._iteration_result(self._iteration_dev(x))",
        "self.outs=self.tr._iteration_dev(self.static_x)"], calls


class _FakeGraph:
    made = []

    def __init__(self):
        _FakeGraph.made.append(self)


class _FakeCapture:
    """Stand-in for torch.cuda.graph: remembers how it was opened and closed, swallows nothing."""
    log = []

    def __init__(self, graph, **kw):
        self.graph, self.kw = graph, kw

    def __enter__(self):
        _FakeCapture.log.append(("enter", self.graph, self.kw))

    def __exit__(self, et, ev, tb):
        _FakeCapture.log.append(("exit", self.graph, et))
        return False


def test_a_capture_that_raises_drops_every_cache_and_a_successful_one_keeps_them_alive(monkeypatch):
    """graphs.capture, rule 5: an fn that fills a registered cache, queues a deferred weight gradient and then raises - the
    same exception comes out, every registered cache and the deferred weight-gradient queues are empty afterwards (their
    tensors would live in the abandoned pool, never written).  Rule 4: a capture that succeeds returns a keepalive that holds
    what fn cached.  torch.cuda.CUDAGraph / torch.cuda.graph / the stream calls of warm_up are stand-ins: no GPU."""
    from dvg_amd import _derived, graphs
    from dvg_amd import autograd as ag

    class FakeStream:
        def wait_stream(self, other):
            pass
    monkeypatch.setattr(_FakeGraph, "made", [])
    monkeypatch.setattr(_FakeCapture, "log", [])
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", _FakeCapture)
    monkeypatch.setattr(torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(graphs, "_streams", {})
    graphs.drop_version_keyed_caches()
    conv = torch.nn.Conv2d(2, 3, 3)
    cached = []

    def fill():
        cached.append(_derived.derived(conv, "t", (conv.weight,), lambda: torch.zeros(3)))
        z = _derived.zero_state(2, 3, torch.device("cpu"))
        return z
    calls = []
    assert graphs.warm_up(lambda: calls.append(1) or len(calls), times=3) == 3 and calls == [1, 1, 1]
    assert graphs.warm_up(fill) is _derived.zero_state(2, 3, torch.device("cpu"))

    class Boom(RuntimeError):
        pass
    boom = Boom("out of memory for the private pool")

    def failing():
        fill()
        ag._wgrad_queues["k"] = [object()]
        ag._dense_queues["k"] = [object()]
        ag._wgrad_flush_queued = True
        raise boom
    with pytest.raises(Boom) as info:
        graphs.capture(failing)
    assert info.value is boom
    assert [e[0] for e in _FakeCapture.log] == ["enter", "exit"] and _FakeCapture.log[1][2] is Boom
    assert _FakeCapture.log[0][2] == {"capture_error_mode": "thread_local"} == graphs.CAPTURE_KW
    assert len(_derived._store) == 0 and len(_derived._zero_states) == 0
    assert _derived.snapshot() == [] and graphs.snapshot_eager_caches() == []
    assert not ag._wgrad_queues and not ag._dense_queues and ag._wgrad_flush_queued is False
    # the context-manager form alone (SegmentedIteration's segments): the same on a raise, the shared pool handed on
    with pytest.raises(Boom):
        with graphs.capturing(pool="POOL") as g:
            assert g is _FakeGraph.made[-1] and _FakeCapture.log[-1] == ("enter", g, {"capture_error_mode": "thread_local", "pool": "POOL"})
            failing()
    assert _derived.snapshot() == [] and not ag._wgrad_queues and ag._wgrad_flush_queued is False
    assert graphs.CAPTURE_KW == {"capture_error_mode": "thread_local"}          # (not written to)
    # a capture that succeeds: graph, result, and a keepalive that holds the tensors fn cached
    del cached[:]
    g, out, keep = graphs.capture(fill)
    assert g is _FakeGraph.made[-1] and _FakeCapture.log[-1] == ("exit", g, None)
    assert out is _derived.zero_state(2, 3, torch.device("cpu"))
    assert {id(cached[0]), id(out)} <= {id(t) for t in keep}
    graphs.drop_version_keyed_caches()
    assert any(t is cached[0] for t in keep) and _derived.snapshot() == []       # the holder's references outlive the caches


def test_skip_scope_clears_around_a_group_and_drops_what_one_capture_added():
    """graphs.skip_scope, rule 2: the skip-keyed caches are empty on entry and after exit; inside, entries stay from one
    capture to the next, and drop_since(mark) forgets exactly the keys added after the mark (GraphedSampler: what the
    posterior graph added goes, what the conditioning graph added stays)."""
    from dvg_amd import _derived, fused, graphs, ops
    from dvg_amd.ops import edge
    dicts = (fused._skip_seen, fused._frozen, edge._SKIP_PROJ_CACHE)
    assert all(any(d is k for k in _derived._skip_keyed) for d in dicts) and len(_derived._skip_keyed) == 3
    a, b = torch.zeros(1), torch.zeros(1)
    fused.declare_frozen_skips([a])
    edge._SKIP_PROJ_CACHE[id(a)] = "eager"
    with graphs.skip_scope() as skips:
        assert not any(dicts)
        fused.declare_frozen_skips([a])
        fused._skip_seen[(1, id(a))] = "cond"
        mark = skips.mark()
        fused.declare_frozen_skips([b])
        fused._skip_seen[(1, id(b))] = "post"
        edge._SKIP_PROJ_CACHE[id(b)] = "post"
        skips.drop_since(mark)
        assert set(fused._frozen) == {id(a)} and fused._skip_seen == {(1, id(a)): "cond"} and not edge._SKIP_PROJ_CACHE
        skips.drop_since(mark)
        assert set(fused._frozen) == {id(a)}
    assert not any(dicts)
    with pytest.raises(KeyError):
        with graphs.skip_scope():
            fused.declare_frozen_skips([a])
            raise KeyError("x")
    assert not any(dicts)
    assert ops.clear_skip_proj_cache is edge.clear_skip_proj_cache
