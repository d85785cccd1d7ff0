"""The exchange schedule of a training step through the module surface (dp.LocalSchedule / AllReduceSchedule /
ShardedSchedule): which one a model gets, and - on two gloo ranks over the emulated engine of tests/test_accum_cpu.py - the
exact sequence of data-parallel and engine calls each of them makes per optimizer step."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import autoencoder_model as ae, dp, model as M, optim
from tests.test_accum_cpu import LR, MIN_USAGE, _micro, _surface
from tests.test_dp_gloo import _free_port, _tiny

# every DataParallel method that launches, waits or communicates (the pure queries - _split, _regions, grad_scale,
# moments_complete - are left out), and the engine methods a step is made of
DP_CALLS = ("train_step", "train_step_sharded", "backward_allreduce", "allreduce_kl", "allreduce_grads", "allreduce_ema",
            "allreduce_ema_async", "_reduce_region", "backward_exchange", "abandon_exchange", "optimizer_step", "forward",
            "finish", "restart_codes", "eval_finish", "sync_optimizer_state", "broadcast_params")
ENG_CALLS = ("forward", "backward", "accum_stats", "accum_grads", "restart_codes", "grad_norm_step", "adam_step", "ratio_step")
CASES = [(s, k) for s in ("local", "allreduce", "sharded") for k in (1, 2)]
STEPS = 2


def _record(obj, names, prefix, trace):
    """Wrap the methods on the INSTANCE, as tests and tools do after attach(): the product has to look them up at call time."""
    for name in names:
        def wrap(inner, label=prefix + name):
            return lambda *a, **kw: (trace.append(label), inner(*a, **kw))[1]
        setattr(obj, name, wrap(getattr(obj, name)))


def _trace(schedule, k, rank, world):
    model, eng = _surface(k, codebook_restart=dict(every=1, min_usage=MIN_USAGE))
    trace, scale = [], 1.0
    _record(eng, ENG_CALLS, "eng.", trace)
    if schedule != "local":
        d = dp.DataParallel()
        d.attach(model, sharded=schedule == "sharded")
        _record(d, DP_CALLS, "dp.", trace)
        model._ema_allreduce = d.allreduce_ema_async if schedule == "sharded" else d.allreduce_ema
        scale = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
    opt = optim.FusedAdam(model, lr=LR, grad_scale=scale, max_grad_norm=0.01, track_update_ratio=True, ema_decay=0.9)
    mbs = _micro(eng, world * k * STEPS)[rank * k * STEPS:(rank + 1) * k * STEPS]
    for mb in mbs:
        opt.zero_grad()
        trace.append("run")
        loss = model.run(*mb)[2]
        trace.append("backward")
        loss.backward()
        trace.append("step")
        opt.step()
        trace.append("state %d %d %d %d" % (model._micro, model._group_ready, model._fold_open, model._grads_cleared))
    assert eng.step_count == STEPS
    return trace


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)                                # (tiny tensors, two processes: more threads only contend)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, {case: _trace(*case, rank, world) for case in CASES}))
    finally:
        dist.destroy_process_group()


# What the commit BEFORE the schedule objects existed does, recorded by running exactly this recorder (_trace) on it - the
# lists below were never taken from the code they check.  One entry per case: the calls of one optimizer step; every step
# of a run repeats them.  "run" / "backward" / "step" mark the surface call the names behind them were made inside of;
# "state m r f c" is (model._micro, _group_ready, _fold_open, _grads_cleared) behind the step.
PARENT = {
    ("local", 1): [
        "run", "eng.forward",
        "backward", "eng.backward", "eng.restart_codes",
        "step", "eng.adam_step", "eng.grad_norm_step", "eng.ratio_step", "state 0 0 0 0"],
    ("local", 2): [
        "run", "eng.forward", "eng.accum_stats",
        "backward", "eng.backward", "eng.accum_grads",
        "step", "state 1 0 0 0",
        "run", "eng.forward", "eng.accum_stats",
        "backward", "eng.backward", "eng.accum_grads", "eng.restart_codes",
        "step", "eng.adam_step", "eng.grad_norm_step", "eng.ratio_step", "state 0 0 0 0"],
    ("allreduce", 1): [
        "run", "dp.finish", "eng.forward", "dp.allreduce_ema",
        "backward", "dp.allreduce_kl", "eng.backward", "dp.restart_codes", "eng.restart_codes", "dp.allreduce_grads",
        "step", "eng.adam_step", "eng.grad_norm_step", "eng.ratio_step", "state 0 0 0 0"],
    ("allreduce", 2): [
        "run", "dp.finish", "eng.forward", "eng.accum_stats",
        "backward", "dp.allreduce_kl", "eng.backward", "eng.accum_grads",
        "step", "state 1 0 0 0",
        "run", "dp.finish", "eng.forward", "eng.accum_stats", "dp.allreduce_ema",
        "backward", "dp.allreduce_kl", "eng.backward", "eng.accum_grads", "dp.restart_codes", "eng.restart_codes",
        "dp.allreduce_grads",
        "step", "eng.adam_step", "eng.grad_norm_step", "eng.ratio_step", "state 0 0 0 0"],
    ("sharded", 1): [
        "run", "dp.forward", "dp.finish", "eng.forward", "dp.finish", "dp.allreduce_ema_async",
        "backward", "dp.backward_exchange", "dp.allreduce_kl", "eng.backward", "dp._reduce_region", "dp._reduce_region",
        "dp.restart_codes", "eng.restart_codes",
        "step", "dp.optimizer_step", "eng.grad_norm_step", "eng.grad_norm_step", "eng.adam_step", "eng.adam_step",
        "eng.adam_step", "eng.ratio_step", "eng.ratio_step", "state 0 0 0 0"],
    ("sharded", 2): [
        "run", "dp.forward", "dp.finish", "eng.forward", "dp.finish", "eng.accum_stats",
        "backward", "dp.allreduce_kl", "eng.backward", "eng.accum_grads",
        "step", "state 1 0 0 0",
        "run", "dp.forward", "dp.finish", "eng.forward", "dp.finish", "eng.accum_stats", "dp.allreduce_ema_async",
        "backward", "dp.backward_exchange", "dp.allreduce_kl", "eng.backward", "eng.accum_grads", "dp._reduce_region",
        "eng.accum_grads", "dp._reduce_region", "dp.restart_codes", "eng.restart_codes",
        "step", "dp.optimizer_step", "eng.grad_norm_step", "eng.grad_norm_step", "eng.adam_step", "eng.adam_step",
        "eng.adam_step", "eng.ratio_step", "eng.ratio_step", "state 0 0 0 0"],
}


@pytest.fixture(scope="module")
def traces():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("schedule,k", CASES, ids=[f"{s}-k{k}" for s, k in CASES])
def test_calls_of_a_step_are_the_parents(traces, schedule, k):
    for rank in (0, 1):
        got = traces[rank][(schedule, k)]
        print(rank, schedule, k, got)
        assert got == PARENT[(schedule, k)] * STEPS, (rank, schedule, k)


class _Group(dp.DataParallel):
    """A DataParallel of any world size without a process group: selection reads world, force_collectives and sharded."""

    def __init__(self, world, force_collectives=False):
        self.world, self.rank, self.group, self.force_collectives = world, 0, None, force_collectives
        self.sharded, self.bf16_grads, self._pending, self._st = False, False, [], None


@pytest.mark.parametrize("world,force,sharded,want", [
    (None, False, False, "LocalSchedule"),                  # no DataParallel attached
    (1, False, False, "LocalSchedule"), (1, False, True, "LocalSchedule"),
    (1, True, False, "AllReduceSchedule"), (1, True, True, "ShardedSchedule"),
    (2, False, False, "AllReduceSchedule"), (2, False, True, "ShardedSchedule"),
    (2, True, False, "AllReduceSchedule"), (2, True, True, "ShardedSchedule")])
def test_selection(world, force, sharded, want):
    model = ae.AutoEncoder(_tiny("vqvae-ema"), n_mel=5)
    if world is None:
        assert type(model._schedule) is dp.LocalSchedule and not model._schedule.shards
        return
    d = _Group(world, force)
    d.attach(model, sharded=sharded)
    sch = model._schedule
    assert type(sch).__name__ == want and type(d.schedule()) is type(sch)
    assert sch.shards is (want == "ShardedSchedule")
    assert want == "LocalSchedule" or sch.dp is d
    # nothing is cached at attach(): what tests and tools set afterwards is seen at the next use
    d.sharded = not sharded
    flipped = {"AllReduceSchedule": "ShardedSchedule", "ShardedSchedule": "AllReduceSchedule"}.get(want, want)
    assert type(model._schedule).__name__ == flipped
    d.force_collectives = not force
    assert (type(model._schedule) is dp.LocalSchedule) == (world == 1 and force)
    model._dp = None
    assert type(model._schedule) is dp.LocalSchedule
