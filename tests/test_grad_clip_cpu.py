"""Global-norm gradient clipping without a GPU: the FusedAdam surface (constructor validation, param_groups,
torch.optim.Adam-format state) and both data-parallel schedules on two gloo ranks, the plans executed by the CPU
interpreter with the clipping handlers of tests/grad_clip_emulator.py."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import checkpoint, config, dp, mfcc_inverter as mi, model as M, optim

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "reference_format.ckpt")


def _model():
    ck = checkpoint.load(CKPT)
    return ck, mi.MfccInverter(config.from_checkpoint_hps(ck["hps"]))


def test_constructor_validation_param_groups_and_state_dict_round_trip():
    ck, m = _model()
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, 1e-3, max_grad_norm=bad)
    assert optim.FusedAdam(m, 1e-3).param_groups[0]["max_grad_norm"] is None          # off unless asked for
    opt = optim.FusedAdam(m, 1e-3, max_grad_norm=2.5)
    assert opt.param_groups[0]["max_grad_norm"] == 2.5
    opt.param_groups[0]["max_grad_norm"] = 0.5                                        # a schedule may change it ...
    assert opt.state_dict()["param_groups"][0]["max_grad_norm"] == 0.5
    opt.param_groups[0]["max_grad_norm"] = -1.0                                       # ... but not to nonsense
    m._engine = object()
    with pytest.raises(ValueError):
        opt.step()
    m._engine = None
    opt.param_groups[0]["max_grad_norm"] = 0.5
    # the state stays in torch.optim.Adam's format: the reference's restore path reads it (tests/test_checkpoint.py)
    checkpoint.restore(m, opt, ck)
    sd = opt.state_dict()
    params = [torch.nn.Parameter(torch.empty_like(p)) for p in m.parameters()]
    stock = torch.optim.Adam(params)
    stock.load_state_dict(sd)
    for i, p in enumerate(params):
        assert float(stock.state[p]["step"]) == 2.0
        assert torch.equal(stock.state[p]["exp_avg"], ck["optim"]["state"][i]["exp_avg"])
        assert torch.equal(stock.state[p]["exp_avg_sq"], ck["optim"]["state"][i]["exp_avg_sq"])
    # a checkpoint WITHOUT the key (torch.optim.Adam's own) loads and leaves the constructor's value alone; one with it sets it
    opt2 = optim.FusedAdam(m, 1e-3, max_grad_norm=3.0)
    opt2.load_state_dict(ck["optim"])
    assert "max_grad_norm" not in ck["optim"]["param_groups"][0] and opt2.param_groups[0]["max_grad_norm"] == 3.0
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["max_grad_norm"] == 0.5
    o2 = opt2.state_dict()
    for i in sd["state"]:
        assert torch.equal(o2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
    # no clipping: the dictionary is what it was before the option existed
    assert "max_grad_norm" not in optim.FusedAdam(m, 1e-3).state_dict()["param_groups"][0]


# ----------------------------------------------------------------------------------------------
# two gloo ranks, both schedules, two clipped steps == ONE process on the global batch with the same clipping
# ----------------------------------------------------------------------------------------------
MAX_NORM = 0.05            # far below the first steps' gradient norms of the tiny model (asserted: the coefficient is < 1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _clip_worker(rank, world, port, bn, q, wg):
    from tests.grad_clip_emulator import emulate_clip
    from tests.test_dp_gloo import _global_batch, _seed_engine, _tiny
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny(bn)
        eng = emulate_clip(M.TrainEngine(hps, B=1, device="cpu", n_mel=5, wgrad_group=wg))
        d = dp.DataParallel()
        batch = _global_batch(eng.geom, 5, world)
        mine = [t[rank:rank + 1] for t in batch]
        gs = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
        n = eng.ps.numel
        out = {}
        for name in ("allreduce", "sharded"):
            _seed_engine(eng)
            eng.clip_out.zero_()
            eng.set_inputs(*mine)
            words = []
            for it in range(2):
                if name == "allreduce":
                    d.train_step(eng, 1e-2, gs, max_grad_norm=MAX_NORM)
                else:
                    d.train_step_sharded(eng, 1e-2, gs, max_grad_norm=MAX_NORM)
                words.append(eng.grad_norm().numpy().copy())
            d.finish()
            if name == "sharded":
                d.gather_moments(eng)
            out[name] = (eng.ps.params[:n].numpy().copy(), eng.adam_m[:n].numpy().copy(), words)
        ref = None
        if rank == 0:
            one = emulate_clip(M.TrainEngine(hps, B=world, device="cpu", n_mel=5))
            _seed_engine(one)
            one.set_inputs(*batch)
            words = []
            for it in range(2):
                one.forward(); one.backward(); one.adam_step(1e-2, 1.0, max_grad_norm=MAX_NORM)
                words.append(one.grad_norm().numpy().copy())
            ref = (one.ps.params[:n].numpy().copy(), one.adam_m[:n].numpy().copy(), words)
        q.put((rank, out, ref))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bn,wg", [("ae", None), ("vqvae-ema", 1)])
def test_dp_clipped_steps_match_single_process_global_batch(bn, wg):
    """Mean-type loss (grad_scale = 1 / world enters the norm) with two exchanged regions, and sum-type loss with three
    (wg = 1: the upper decoder layers' region has its own shard layout).  The tolerances are those of
    tests/test_dp_gloo.py::test_dp_real_steps_match_single_process_global_batch for the unclipped step."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_clip_worker, args=(r, world, port, bn, q, wg)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, o0, ref), (_, o1, _) = res
    T = torch.from_numpy
    p_ref, m_ref, w_ref = T(ref[0]), T(ref[1]), ref[2]
    scale = float(p_ref.abs().max())
    for it in range(2):
        assert 0.0 < w_ref[it][1] < 1.0 and w_ref[it][2] == 0.0 and w_ref[it][3] == 0.0, w_ref[it]    # the clip is active
    for name in ("allreduce", "sharded"):
        (pa, ma, wa), (pb, mb, wb) = o0[name], o1[name]
        pa, ma, pb, mb = T(pa), T(ma), T(pb), T(mb)
        for it in range(2):
            assert wa[it].tobytes() == wb[it].tobytes(), (name, it, wa[it], wb[it])   # one coefficient on every rank, bit for bit
            assert abs(wa[it][0] / w_ref[it][0] - 1) < 2e-5 and abs(wa[it][1] / w_ref[it][1] - 1) < 2e-5, (name, wa[it], w_ref[it])
            assert wa[it][2] == 0.0 and wa[it][3] == 0.0
        assert torch.equal(pa, pb) and torch.equal(ma, mb), name                      # the replicas stay identical
        assert float((pa - p_ref).abs().max()) <= 2e-5 * scale, (name, float((pa - p_ref).abs().max()), scale)
        assert float((ma - m_ref).abs().max()) <= 2e-5 * max(float(m_ref.abs().max()), 1e-12), name
