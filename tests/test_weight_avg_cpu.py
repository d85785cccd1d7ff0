"""Averaged (EMA) weights without a GPU: the FusedAdam surface (constructor validation, param_groups, the decay schedule,
torch.optim.Adam-format state with `param_avg` beside `exp_avg`) and the sharded data-parallel schedule on two gloo
ranks, the plans executed by the CPU interpreter with the handlers of tests/weight_avg_emulator.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import checkpoint, config, dp, mfcc_inverter as mi, model as M, optim
from tests.test_update_ratio_cpu import _free_port

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "reference_format.ckpt")
ADAM_GROUP_KEYS = {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
                   "fused", "params"}


def _model():
    ck = checkpoint.load(CKPT)
    return ck, mi.MfccInverter(config.from_checkpoint_hps(ck["hps"]))


def test_constructor_validation_param_groups_and_state_dict_keys():
    ck, m = _model()
    for bad in (0, 1, -0.1, "x", 0.0, 1.0, 1.5, float("nan"), True, [0.5, 0.5]):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, 1e-3, ema_decay=bad)
    for bad in (None, "yes", 2):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, 1e-3, ema_decay=0.9, ema_warmup=bad)
    plain = optim.FusedAdam(m, 1e-3)
    assert plain.param_groups[0]["ema_decay"] is None               # off unless asked for
    opt = optim.FusedAdam(m, 1e-3, ema_decay=0.999)
    assert opt.param_groups[0]["ema_decay"] == 0.999 and opt.param_groups[0]["ema_warmup"] is True
    assert optim.FusedAdam(m, 1e-3, ema_decay=0.5, ema_warmup=False).param_groups[0]["ema_warmup"] is False
    for ok in (np.float32(0.75), np.float64(0.75), torch.tensor(0.75)):      # whatever float() takes, like max_grad_norm
        assert optim.FusedAdam(m, 1e-3, ema_decay=ok).param_groups[0]["ema_decay"] == 0.75
    with pytest.raises(L.AewError):                                 # no engine, no averaged step
        with opt.averaged_weights():
            pass
    opt.param_groups[0]["ema_decay"] = 1.0                          # a schedule may change it, but not to nonsense
    m._engine = object()
    with pytest.raises(ValueError):
        opt.step()
    m._engine = None
    opt.param_groups[0]["ema_decay"] = 0.999
    # off: the dictionary is what it was before the option existed - key sets and the group itself
    checkpoint.restore(m, plain, ck)
    sd_plain = plain.state_dict()
    assert set(sd_plain["param_groups"][0]) == ADAM_GROUP_KEYS
    assert sd_plain["param_groups"][0] == {
        "lr": plain.param_groups[0]["lr"], "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False,
        "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
        "params": list(range(len(list(m.parameters()))))}
    assert len(sd_plain["state"]) > 0
    for s in sd_plain["state"].values():
        assert set(s) == {"step", "exp_avg", "exp_avg_sq"}
    # on: three extra group keys that torch.optim.Adam carries along; no average yet, so no param_avg and avg_steps = 0
    checkpoint.restore(m, opt, ck)
    sd = opt.state_dict()
    g = sd["param_groups"][0]
    assert set(g) == ADAM_GROUP_KEYS | {"ema_decay", "ema_warmup", "avg_steps"}
    assert (g["ema_decay"], g["ema_warmup"], g["avg_steps"]) == (0.999, True, 0)
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    stock = torch.optim.Adam([torch.nn.Parameter(torch.empty_like(p)) for p in m.parameters()])
    stock.load_state_dict(sd)
    # together with the other options
    both = optim.FusedAdam(m, 1e-3, max_grad_norm=2.0, track_update_ratio=True, ema_decay=0.9).state_dict()["param_groups"][0]
    assert both["max_grad_norm"] == 2.0 and both["track_update_ratio"] is True and both["ema_decay"] == 0.9


@pytest.mark.parametrize("decay", [0.9, 0.999, 0.9999])
def test_decay_schedule_against_the_closed_form(decay):
    for t in range(201):
        want = min(decay, (1.0 + t) / (10.0 + t))
        assert optim.ema_decay_at(decay, t, True) == want
        assert optim.ema_decay_at(decay, t, False) == decay
        for warm, d in ((True, want), (False, decay)):
            r = optim.ema_rate_at(decay, t, warm)
            assert r == float(np.float32(1.0 - d)) and np.float32(r) == r     # the fp32 rounding of the double, once
            assert 0.0 < r < 1.0
    assert optim.ema_decay_at(decay, 0, True) == 0.1                 # the first averaged step mostly takes the new weights
    assert optim.ema_decay_at(decay, 10 ** 6, True) == decay         # ... and the warm-up ends


def test_state_dict_round_trip_with_and_without_the_average():
    ck, m = _model()
    opt = optim.FusedAdam(m, 1e-3, ema_decay=0.99, ema_warmup=False)
    checkpoint.restore(m, opt, ck)
    sd = opt.state_dict()
    gen = torch.Generator().manual_seed(9)
    for s in sd["state"].values():                                  # a checkpoint written after 5 averaged steps
        s["param_avg"] = torch.randn(s["exp_avg"].shape, generator=gen)
    sd["param_groups"][0]["avg_steps"] = 5
    opt.load_state_dict(sd)
    out = opt.state_dict()
    # ... through a fresh model and an optimizer built without averaging: the checkpoint switches it on
    _, m2 = _model()
    opt2 = optim.FusedAdam(m2, 1e-3)
    opt2.load_state_dict(out)
    out2 = opt2.state_dict()
    for o in (out, out2):
        g = o["param_groups"][0]
        assert (g["ema_decay"], g["ema_warmup"], g["avg_steps"]) == (0.99, False, 5)
        assert len(o["state"]) == len(sd["state"])
        for i, s in sd["state"].items():
            assert set(o["state"][i]) == {"step", "exp_avg", "exp_avg_sq", "param_avg"}
            for k in ("exp_avg", "exp_avg_sq", "param_avg"):
                assert torch.equal(o["state"][i][k], s[k]), (i, k)
            assert float(o["state"][i]["step"]) == float(s["step"])
    c = m2._opt_carry
    assert c.avg_steps == 5 and c.averaged_in is False and c.step == 2 and c.avg is not None and c.complete is True
    assert c._fields == ("step", "m", "v", "avg_steps", "avg", "averaged_in", "complete")
    # torch.optim.Adam reads the dictionary (extra keys travel along)
    stock = torch.optim.Adam([torch.nn.Parameter(torch.empty_like(p)) for p in m.parameters()])
    stock.load_state_dict(out)
    # a reference-format checkpoint without the keys still loads: the constructor's options stay, and there is no average
    # any more - it starts again at the next step
    opt2.load_state_dict(ck["optim"])
    assert "ema_decay" not in ck["optim"]["param_groups"][0]
    assert opt2.param_groups[0]["ema_decay"] == 0.99 and m2._opt_carry.avg is None
    o3 = opt2.state_dict()
    assert o3["param_groups"][0]["avg_steps"] == 0
    for i, s in ck["optim"]["state"].items():
        assert set(o3["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.equal(o3["state"][i]["exp_avg"], s["exp_avg"])
    # an average for some parameters only is refused
    del out["state"][0]["param_avg"]
    with pytest.raises(ValueError):
        opt2.load_state_dict(out)


# ----------------------------------------------------------------------------------------------
# two gloo ranks, sharded schedule, three averaged steps == ONE process on the global batch
# ----------------------------------------------------------------------------------------------
DECAY, STEPS = 0.9, 3


def _avg_worker(rank, world, port, q):
    from ae_wavenet_amd import autoencoder_model as ae
    from tests.test_dp_gloo import _global_batch, _seed_engine, _tiny
    from tests.weight_avg_emulator import avg_update, emulate_avg
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny("vqvae-ema")
        torch.manual_seed(5)
        model = ae.AutoEncoder(hps, n_mel=5)
        eng = emulate_avg(M.TrainEngine(hps, B=1, device="cpu", n_mel=5, wgrad_group=1))
        model._adopt_engine(eng)
        d = dp.DataParallel()
        d.attach(model, sharded=True)
        opt = optim.FusedAdam(model, lr=1e-2, ema_decay=DECAY)
        batch = _global_batch(eng.geom, 5, world)
        _seed_engine(eng)
        eng.set_inputs(*[t[rank:rank + 1] for t in batch])
        gs = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
        n = eng.ps.numel
        want = eng.ps.params[:n].numpy().copy()                     # the average starts from the weights in front of step 1
        for it in range(STEPS):
            rate = optim.ema_rate_at(DECAY, eng.avg_steps)
            d.train_step_sharded(eng, 1e-2, gs, avg_rate=rate)
            d.finish()
            want = avg_update(want, rate, eng.ps.params[:n].numpy())   # numpy recursion over this rank's own parameters
        mine = eng.adam_avg[:n].numpy().copy()
        raised = False
        try:
            with opt.averaged_weights():
                pass
        except L.AewError as e:
            raised = "sync_optimizer_state" in str(e)
        untouched = not eng.averaged_in and np.array_equal(eng.adam_avg[:n].numpy(), mine)
        d.sync_optimizer_state(model)
        full = eng.adam_avg[:n].numpy().copy()
        p_raw = eng.ps.params[:n].numpy().copy()
        with opt.averaged_weights():                                # complete now: the swap goes through and comes back
            inside = eng.ps.params[:n].numpy().copy()
        back = np.array_equal(eng.ps.params[:n].numpy(), p_raw) and np.array_equal(eng.adam_avg[:n].numpy(), full)
        ref = None
        if rank == 0:
            one = emulate_avg(M.TrainEngine(hps, B=world, device="cpu", n_mel=5))
            _seed_engine(one)
            one.set_inputs(*batch)
            for it in range(STEPS):
                one.forward(); one.backward()
                one.adam_step(1e-2, 1.0, avg_rate=optim.ema_rate_at(DECAY, one.avg_steps))
            ref = (one.adam_avg[:n].numpy().copy(), one.ps.params[:n].numpy().copy())
        q.put((rank, raised, untouched, mine, full, want, inside, back, p_raw, eng.avg_steps, ref))
    finally:
        dist.destroy_process_group()


def test_sharded_average_is_complete_after_the_sync_and_matches_a_single_process():
    """Three sharded steps with wg = 1 (three exchanged regions: shard cuts fall inside tensors).  Each rank averages its
    own shards and the replicated remainders; after sync_optimizer_state every rank holds the whole average: bit for bit
    the numpy recursion over its own parameters (equal parameters give equal averages), bit for bit the other rank's, and
    against one process on the global batch within the bound tests/test_dp_gloo.py holds the parameters to (the
    gradients of the two runs differ in summation order).  The recursion is weight_avg_emulator.avg_update, the function
    the interpreter's Adam handler itself uses: the bit equality checks the sharding, the range calls and the gather, NOT
    the kernel's formula - that is held to an independent numpy restatement by tests/test_weight_avg_gpu.py only."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_avg_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref_avg, ref_p = res[0][10]
    for rank, raised, untouched, mine, full, want, inside, back, p_raw, avg_steps, _ in res:
        assert raised and untouched, rank                           # before the sync: refused, nothing swapped
        assert avg_steps == STEPS
        assert not np.array_equal(mine, full), "each rank really was missing the other's shards"
        assert full.tobytes() == want.tobytes(), rank               # complete, and the kernel's recursion bit for bit
        assert inside.tobytes() == full.tobytes() and back, rank
        assert not np.array_equal(full, p_raw)
        scale = float(np.abs(ref_p).max())
        assert np.abs(p_raw - ref_p).max() <= 2e-5 * scale
        assert np.abs(full - ref_avg).max() <= 2e-5 * scale, (rank, np.abs(full - ref_avg).max(), scale)
    assert res[0][4].tobytes() == res[1][4].tobytes()               # the ranks hold the same average


# ----------------------------------------------------------------------------------------------
# the optimizer state as one record (model.OptState): out of one engine, into another
# ----------------------------------------------------------------------------------------------
def test_opt_state_record_moves_everything_between_engines():
    """Engine A (B = 1) takes two averaged steps and swaps the average in; its record, cloned, goes into engine B (B = 2:
    other plans, the same flat layout).  B then holds A's state bit for bit, refuses to step like A, and after swapping
    back takes the third step exactly as a twin of A does whose state never moved.  adam_step reads the gradient buffer
    alone, so the three gradients are written there: no forward / backward, and the batch size does not matter."""
    from tests.test_dp_gloo import _seed_engine, _tiny
    from tests.weight_avg_emulator import emulate_avg
    hps = _tiny("vqvae-ema")
    a, twin = (emulate_avg(M.TrainEngine(hps, B=1, device="cpu", n_mel=5)) for _ in range(2))
    b = emulate_avg(M.TrainEngine(hps, B=2, device="cpu", n_mel=5))
    n = a.ps.numel
    assert b.ps.numel == n
    grads = [torch.randn(n, generator=torch.Generator().manual_seed(20 + i)) for i in range(3)]
    bits = lambda t: t.numpy().tobytes()

    def step(eng, i):
        eng.ps.grads[:n].copy_(grads[i])
        eng.adam_step(1e-2, 1.0, avg_rate=optim.ema_rate_at(DECAY, eng.avg_steps))

    for eng in (a, twin):
        _seed_engine(eng)
        step(eng, 0)
        step(eng, 1)
    a.swap_averaged()
    st = a.opt_state(clone=True)
    assert st._fields == ("step", "m", "v", "avg_steps", "avg", "averaged_in", "complete")
    assert st.m.data_ptr() != a.adam_m.data_ptr() and st.avg.data_ptr() != a.adam_avg.data_ptr()      # clones ...
    b.ps.params[:n].copy_(a.ps.params[:n])                          # (the parameters move beside the record)
    b.load_opt_state(st)
    got, want = b.opt_state(clone=False), a.opt_state(clone=False)
    assert got.m.data_ptr() == b.adam_m.data_ptr() and got.avg.data_ptr() == b.adam_avg.data_ptr()    # ... and views
    assert (got.step, got.avg_steps, got.averaged_in, got.complete) == (2, 2, True, True)
    assert (want.step, want.avg_steps, want.averaged_in, want.complete) == (2, 2, True, True)
    for f in ("m", "v", "avg"):
        assert bits(getattr(got, f)) == bits(getattr(want, f)), f
    assert bits(got.avg) != bits(b.ps.params[:n]) and float(got.m.abs().max()) > 0
    for eng in (a, b):                                              # swapped in: no step, and nothing counted
        with pytest.raises(L.AewError):
            step(eng, 2)
        assert (eng.step_count, eng.avg_steps) == (2, 2)
    b.swap_averaged()
    assert not b.averaged_in
    step(b, 2)
    step(twin, 2)
    assert (b.step_count, b.avg_steps) == (twin.step_count, twin.avg_steps) == (3, 3)
    for f in ("adam_m", "adam_v", "adam_avg"):
        assert bits(getattr(b, f)[:n]) == bits(getattr(twin, f)[:n]), f
    assert bits(b.ps.params[:n]) == bits(twin.ps.params[:n])
    # a record without an average leaves an engine that holds one without
    b.load_opt_state(st._replace(avg=None))
    assert b.avg_live is False and b.avg_steps == 0 and b.averaged_in is False and b.step_count == 2
    assert b.opt_state(clone=False).avg is None and len(b.opt_buffers()) == 2
