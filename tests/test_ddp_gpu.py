"""GPU: the data-parallel training step with two ranks (gloo rendezvous, both ranks on cuda:0 - RCCL needs one GPU per rank, the
collective semantics are the same): after a full curriculum cycle on different author shards the replicated weights of the two
ranks must still be identical, and must differ from a single-rank run (i.e. the exchange really happened)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, out, workdir):
    import random
    import faulthandler
    faulthandler.dump_traceback_later(420, exit=False)     # a rank that hangs says where (the parent gives up after 600 s and retries once)
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_gan_trainer
    rng.set_mode("device", seed=7 + rank)
    torch.manual_seed(0)   # same initial weights on every rank
    wd = os.path.join(workdir, "r%d" % rank)
    os.makedirs(wd, exist_ok=True)
    trainer, _ = build_gan_trainer("iam_gan", 1, 2, width=256, label_len=12, workdir=wd, rank=rank, world=world)
    torch.manual_seed(100 + rank); np.random.seed(100 + rank); random.seed(100 + rank)
    for it in range(7):
        trainer._train_iteration(it)
    torch.cuda.synchronize()
    digest = torch.stack([p.detach().double().sum() for p in trainer.model.parameters()]).cpu()
    finite = bool(torch.isfinite(digest).all())
    out[(world, rank)] = (digest.tolist(), finite)
    if world > 1:
        dist.destroy_process_group()


def _run(world, tmp):
    """The ranks share ONE GPU and talk gloo here (RCCL wants a GPU per rank) - a harness the product never runs in. Once in ~8 full-suite runs of
    round 6 a rank of this harness sat in a collective until the 600 s limit with no exception on either side (the same code passed before and
    after on other boxes). A rank that HANGS is therefore retried once, loudly (the hung rank dumps its stacks through faulthandler first); a
    rank that exits non-zero, or a second hang, fails the test."""
    for attempt in (0, 1):
        ctx = mp.get_context("spawn")
        mgr = ctx.Manager()
        out = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, world, port, out, tmp)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        codes = [p.exitcode for p in procs]
        for p in procs:
            if p.exitcode is None:
                p.kill()
        hung = any(c is None for c in codes)
        if hung and attempt == 0:
            print("tests/test_ddp_gpu.py: a rank hung (exit codes %s); retrying once" % (codes,), flush=True)
            continue
        assert codes == [0] * world, codes
        return dict(out)


def test_two_ranks_keep_identical_weights(cuda, tmp_path):
    two = _run(2, str(tmp_path))
    d0, ok0 = two[(2, 0)]
    d1, ok1 = two[(2, 1)]
    assert ok0 and ok1, "non-finite parameters after the cycle"
    assert d0 == d1, "replicated weights diverged between the ranks: max |diff| %.3e" % max(abs(a - b) for a, b in zip(d0, d1))
    one = _run(1, str(tmp_path / "single"))
    s0, _ = one[(1, 0)]
    assert any(abs(a - b) > 1e-9 for a, b in zip(s0, d0)), "two-rank run equals the single-rank run: no gradient exchange happened"


# ---------------------------------------------------------------------------------------------------------------------------------
# N ranks == one process that runs the N author shards one after the other on the same weights and averages every gradient set
# ("semantics to pin"), at the per-GPU shape of BASELINE configs[3]: 4 authors x 2 lines of 64 x 512.
def _digest(trainer):
    return {k: p.detach().double().cpu() for k, p in trainer.model.named_parameters()}


def _grad_fingerprints(trainer):
    """per parameter: None, or [sum |g|, sum g^2, projection on a fixed cosine vector] of the gradient about to be clipped"""
    f = trainer.flat
    pos_of = {id(f.params[pi]): k for k, pi in enumerate(f.order)}
    out, rows, keys = {}, [], []
    for j, (n, p) in enumerate(trainer.model.named_parameters()):
        if not f.touched[pos_of[id(p)]]:
            out[n] = None
            continue
        d = p.grad.detach().double().flatten()
        r = torch.cos(torch.arange(d.numel(), dtype=torch.float64, device=d.device) * 0.37 + 1.3 * j)
        rows.append(torch.stack([d.abs().sum(), (d * d).sum(), (d * r).sum()]))
        keys.append(n)
    host = torch.stack(rows).cpu().tolist() if rows else []
    out.update(dict(zip(keys, host)))
    return out


def _dp_worker(rank, world, port, out, workdir, shape):
    import random
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_gan_trainer
    B, A, W, L, iters = shape
    rng.set_mode("device", seed=7 + rank)
    torch.manual_seed(0)
    wd = os.path.join(workdir, "r%d" % rank)
    os.makedirs(wd, exist_ok=True)
    trainer, _ = build_gan_trainer("iam_gan", B, A, width=W, label_len=L, workdir=wd, rank=rank, world=world)
    torch.manual_seed(100 + rank); np.random.seed(100 + rank); random.seed(100 + rank)
    logs, grads = [], {}
    trainer.pre_clip_hook = lambda it: grads.__setitem__(it, _grad_fingerprints(trainer))
    for it in range(iters):
        logs.append(trainer._train_iteration(it))
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"params": _digest(trainer), "logs": logs, "grads": grads}, os.path.join(workdir, "dp.pt"))
    out[rank] = True
    dist.destroy_process_group()


def _sequential_worker(world, out, workdir, shape):
    """one process, `world` virtual ranks: each has its own author shard, host RNG streams, device Philox stream and style bank; the
    non-trainable state every real rank would see (spectral-norm u / v, BatchNorm running statistics) is rewound between the shards"""
    import random
    import numpy as np
    torch.set_num_threads(1)
    from handwriting_line_generation_amd import ops, rng
    from handwriting_line_generation_amd.data.synthetic import SyntheticLoader
    from handwriting_line_generation_amd.harness import build_gan_trainer
    B, A, W, L, iters = shape
    torch.manual_seed(0)
    wd = os.path.join(workdir, "seq")
    os.makedirs(wd, exist_ok=True)
    trainer, _ = build_gan_trainer("iam_gan", B, A, width=W, label_len=L, workdir=wd, rank=0, world=1)
    flat = trainer.flat
    vr = []
    for r in range(world):
        torch.manual_seed(100 + r); np.random.seed(100 + r); random.seed(100 + r)
        vr.append({"torch": torch.get_rng_state(), "np": np.random.get_state(), "py": random.getstate(), "dev": ops.DeviceRNG(7 + r),
                   "styles": [], "loader": iter(SyntheticLoader(trainer.data_loader.dataset, r, world))})
    frozen = [t for t in list(trainer.model.buffers()) + [p for p in trainer.model.parameters() if not p.requires_grad]]
    logs, grads = [], {}
    trainer.pre_clip_hook = lambda it: grads.__setitem__(it, _grad_fingerprints(trainer))
    for it in range(iters):
        trainer.model.train()
        lesson = trainer.curriculum.getLesson(it)
        shared_stashes = list(trainer.saved_grads)          # averaged sets stashed by earlier no-step lessons
        before = [t.detach().clone() for t in frozen]
        # the flat gradient buffer is identical on all ranks at the start of an iteration (everything that was touched has been averaged or
        # stashed away): recogniser gradients, which no optimizer ever zeroes, keep accumulating in it and enter the balancing rule's
        # "tensor with an all-zero gradient" fallback, so every shard must start from this state, not from the previous shard's leftovers
        grad0, touched0 = flat.flat_grad.clone(), flat.touched.copy()
        parts, first = [], None
        for r in range(world):
            for t, b in zip(frozen, before):
                t.data.copy_(b)
            flat.flat_grad.copy_(grad0)
            flat.touched[:] = touched0
            torch.set_rng_state(vr[r]["torch"]); np.random.set_state(vr[r]["np"]); random.setstate(vr[r]["py"])
            rng._state["rng"] = vr[r]["dev"]
            trainer.prev_styles = vr[r]["styles"]
            trainer.data_loader_iter = vr[r]["loader"]
            trainer.saved_grads = []
            instance = trainer._next_instance(lesson)
            produced = trainer._forward_backward(instance, lesson)
            assert produced is not None
            torch.cuda.synchronize()
            parts.append((flat.flat_grad.clone(), flat.touched.copy(), [(s[0].clone(), s[1].copy()) for s in trainer.saved_grads]))
            for s in trainer.saved_grads:
                flat.release(s)
            vr[r].update(torch=torch.get_rng_state(), np=np.random.get_state(), py=random.getstate(), styles=trainer.prev_styles)
            if r == 0:
                first = (instance, produced, [t.detach().clone() for t in frozen])
        # what the all-reduce delivers on every rank: sums divided by the world size, None-masks OR-ed
        flat.flat_grad.copy_(sum(p[0] for p in parts)).div_(world)
        flat.touched[:] = np.logical_or.reduce([p[1] for p in parts])
        new = []
        for k in range(len(parts[0][2])):
            buf = sum(p[2][k][0] for p in parts).div_(world)
            new.append([buf, np.logical_or.reduce([p[2][k][1] for p in parts]), None])
        trainer.saved_grads = shared_stashes + new
        for t, b in zip(frozen, first[2]):
            t.data.copy_(b)
        logs.append(trainer._apply_step(lesson, it, first[0], *first[1]))
    torch.cuda.synchronize()
    torch.save({"params": _digest(trainer), "logs": logs, "grads": grads}, os.path.join(workdir, "seq.pt"))
    out["seq"] = True


def test_two_ranks_equal_sequential_shards_averaged(cuda, tmp_path):
    shape = (4, 2, 512, 30, 7)      # authors, lines per author, width, label length, iterations (one curriculum cycle)
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    out = mgr.dict()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out, str(tmp_path), shape)) for r in range(2)]
    procs.append(ctx.Process(target=_sequential_worker, args=(2, out, str(tmp_path), shape)))
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
        assert p.exitcode == 0
    dp = torch.load(os.path.join(str(tmp_path), "dp.pt"))
    sq = torch.load(os.path.join(str(tmp_path), "seq.pt"))
    # Every kernel is deterministic (no floating-point atomics), but bit-exact agreement is still out of reach: two ranks form
    # (g0 + g1) / 2 in the all-reduce while the sequential run accumulates the shards into one buffer, i.e. a different summation order in
    # the last bit, and Adam's first steps (update = lr * g / (|g| + eps): the SIGN of g) turn a last-bit difference of a near-zero
    # gradient element into a 2 * lr difference of that weight. What is compared is therefore what the data-parallel machinery produces -
    # the averaged, balanced gradient every rank is about to clip, per parameter, with exactly the same tensors present - tightly while
    # the weights are still identical (iterations 0-2: count step, stashing gen lesson, auto lesson balanced from four stashes) and
    # loosely after the first optimizer steps have decorrelated the two trajectories.
    assert sorted(dp["grads"]) == sorted(sq["grads"]) == [0, 2, 3, 5, 6]
    for it in sorted(dp["grads"]):
        ga, gb = dp["grads"][it], sq["grads"][it]
        groups = {}
        for k in ga:
            assert (ga[k] is None) == (gb[k] is None), "iteration %d: gradient of %s present on one side only" % (it, k)
            if ga[k] is None:
                continue
            nrm = max(gb[k][1], 1e-300) ** 0.5
            e = max(abs(ga[k][2] - gb[k][2]) / nrm, abs(ga[k][0] - gb[k][0]) / max(gb[k][0], 1e-300))
            if k.split(".")[0] != "hwr":      # recogniser gradients are never used (frozen) and mostly rounding noise around zero
                groups.setdefault(k.split(".")[0], []).append(e)
        for top, es in groups.items():
            rms = (sum(e * e for e in es) / len(es)) ** 0.5
            assert rms < (2e-5 if it <= 2 else 5e-2), "iteration %d %s: averaged gradients differ by %.2e (rms over %d tensors)" % (it, top, rms, len(es))
    for it, (a, b) in enumerate(zip(dp["logs"], sq["logs"])):      # rank 0's own losses are the first shard's losses
        for k in a:
            tol = 1e-6 if it <= 2 else 2e-2
            assert abs(a[k] - b[k]) <= tol * max(abs(b[k]), 1e-2), "iteration %d %s: 2 ranks %r, sequential %r" % (it, k, a[k], b[k])
    # the weights after the cycle: same updates up to those sign flips
    num = sum(float((v - sq["params"][k]).pow(2).sum()) for k, v in dp["params"].items())
    den = sum(float(v.pow(2).sum()) for v in sq["params"].values())
    assert (num / den) ** 0.5 < 1e-4, "weights after the cycle differ by %.2e relative" % ((num / den) ** 0.5)


def _rccl_worker(force, port, out_path, workdir):
    """one rank, backend nccl (RCCL): a curriculum cycle with (force) or without the data-parallel exchange switched on"""
    import random

    import numpy as np
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HWG_FORCE_DP="1" if force else "0")
    torch.cuda.set_device(0)
    if force:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from handwriting_line_generation_amd import rng
    from handwriting_line_generation_amd.harness import build_gan_trainer
    from handwriting_line_generation_amd.trainer import flat_params
    assert flat_params.FORCE_DP == bool(force)
    torch.manual_seed(0); np.random.seed(0); random.seed(0)
    rng.set_mode("device", seed=7)
    trainer, _ = build_gan_trainer("iam_gan", 2, 2, width=256, label_len=12, workdir=workdir)
    for it in range(7):
        trainer._train_iteration(it)
    torch.cuda.synchronize()
    torch.save({"params": {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()}, "comm": dict(flat_params.COMM)}, out_path)
    if force:
        dist.destroy_process_group()


def test_single_rank_rccl_exchange_is_the_identity(cuda, tmp_path):
    """The RCCL code path itself (backend "nccl": asynchronous whole-buffer reductions of the stashed sets under the following backward passes,
    the int32 MAX exchange of the None-masks, span reductions of the current set, the gloo control group) on the one GPU a test box has: with
    HWG_FORCE_DP=1 a one-rank process group runs every collective of the data-parallel step, and the weights after a curriculum cycle must be
    bit-identical to the plain single-process step."""
    ctx = mp.get_context("spawn")
    outs = []
    for force in (1, 0):
        path = os.path.join(str(tmp_path), "w%d.pt" % force)
        p = ctx.Process(target=_rccl_worker, args=(force, _free_port(), path, str(tmp_path / ("wd%d" % force))))
        p.start(); p.join(900)
        assert p.exitcode == 0
        outs.append(torch.load(path))
    forced, plain = outs
    assert forced["comm"]["collectives"] > 20 and forced["comm"]["bytes"] > 500e6 and plain["comm"]["collectives"] == 0
    for k, v in plain["params"].items():
        assert torch.equal(v, forced["params"][k]), "%s differs after a cycle with the one-rank RCCL exchange" % k


def _bench_two_gloo_ranks(tmp_path, *extra):
    """`bench.py --gpus 2 --steps 7 --warmup 0` as the driver launches it (one process per rank, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from
    the environment), here with HWG_DIST_BACKEND=gloo so that both ranks can share the one GPU of the lease; returns rank 0's JSON line after
    checking that the rank-sharded path (per-rank author shards, gradient-set all-reduces, max-over-ranks timing) reported a 2-rank job"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HWG_DIST_BACKEND="gloo",
                   HWG_BENCH_NO_MINNEC="1", HWG_BENCH_PROF_CYCLES="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "0", "--no-cpu-baseline", "--no-gen",
                                       *extra],
                                      cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    lines = [[l for l in so.splitlines() if l.startswith('{"metric"')] for so, _ in outs]      # (gloo itself chats on stdout)
    assert len(lines[0]) == 1 and lines[1] == [], "ONE JSON line, from rank 0"
    line = json.loads(lines[0][0])
    assert line["n_gpus"] == 2 and line["steps"] == 7 and line["warmup"] == 0 and line["scaling"] == "weak"
    assert line["data_parallel"]["world_size"] == 2 and line["data_parallel"]["backend"] == "gloo"
    assert line["data_parallel"]["collectives_per_step"] > 0 and line["data_parallel"]["allreduce_mbytes_per_step"] > 0
    assert line["value"] > 0 and line["value"] == line["value"] and line["value"] != float("inf")
    assert abs(line["value"] - 2 * 7 / (line["ms_per_step"] * 7e-3)) < 0.01 * line["value"]      # whole-job aggregate: N x K / max-over-ranks time
    return line


def test_bench_rank_sharded_path_with_two_gloo_ranks(cuda, tmp_path):
    """`bench.py --gpus 2 --full` with two gloo ranks on the one GPU: the rank-sharded path and the secondary loops after the timed region that
    every rank runs (whole cycles with their max-over-ranks timing, the profiled cycles with collectives inside) must run and report a 2-rank
    job. Keeps SURVEY 8(e)'s N > 1 bench path from rotting while no multi-GPU node is available to the build."""
    line = _bench_two_gloo_ranks(tmp_path, "--full")
    assert line["other_workloads"] is None


def test_bench_plain_run_with_two_gloo_ranks(cuda, tmp_path):
    """`bench.py --gpus 2` without --full, the driver's launch: the same 2-rank job, and none of the secondary measurements ran"""
    line = _bench_two_gloo_ranks(tmp_path)
    for key in ("whole_cycles", "roofline", "gen_lines_per_sec", "cpu_baseline", "minimum_necessary", "other_workloads", "clocks"):
        assert line[key] is None, key
    assert line["data_parallel"]["rccl"] is None
