"""Per-parameter update / weight ratios without a GPU: the chunk builder (aew_uw_chunks, host logic of the library), the
FusedAdam surface (constructor validation, param_groups, torch.optim.Adam-format state) and both data-parallel
schedules on two gloo ranks, the plans executed by the CPU interpreter with the handlers of
tests/update_ratio_emulator.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import checkpoint, config, dp, mfcc_inverter as mi, model as M, optim

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "reference_format.ckpt")
CH = L.UW_CHUNK
SIZES = [4, 1, 7, CH, CH + 1, 2 * CH + 1, 3]


def padded_offsets(sizes):
    """The ParamStore rule: every tensor starts at a multiple of 4."""
    offs, o = [], 0
    for k in sizes:
        offs.append(o)
        o += (k + 3) // 4 * 4
    return offs, o


def test_chunk_builder_tiles_every_tensor_and_nothing_else():
    offs, total = padded_offsets(SIZES)
    chunks, first = L.uw_chunks(offs, SIZES)
    nch = first[-1]
    assert nch == sum((k + CH - 1) // CH for k in SIZES) and len(first) == len(SIZES) + 1
    owner = np.full(total, -1)
    prev = (-1, -1)
    for c in range(nch):
        off, ln, t = chunks[c].off, chunks[c].len, chunks[c].tensor
        assert 1 <= ln <= CH and off % 4 == 0
        assert offs[t] <= off and off + ln <= offs[t] + SIZES[t], "a chunk crosses a tensor boundary"
        assert (t, off) > prev, "tensors ascending, chunks ascending within a tensor"
        prev = (t, off)
        assert (owner[off:off + ln] == -1).all(), "chunks overlap"
        owner[off:off + ln] = t
        assert first[t] <= c < first[t + 1]
    for t, (o, k) in enumerate(zip(offs, SIZES)):
        assert (owner[o:o + k] == t).all(), "the chunks tile every tensor exactly"
        assert (owner[o + k:(o + k + 3) // 4 * 4] == -1).all(), "pad elements belong to no chunk"
        assert chunks[first[t]].off == o and first[t + 1] - first[t] == (k + CH - 1) // CH
    # a tensor of length 0 has no chunk; misplaced tensors are refused
    _, f0 = L.uw_chunks([0, 8, 8], [5, 0, 3])
    assert f0 == [0, 1, 1, 2]
    with pytest.raises(L.AewError):
        L.uw_chunks([0, 2], [1, 1])                                 # offset not a multiple of 4
    with pytest.raises(L.AewError):
        L.uw_chunks([0, 4], [5, 1])                                 # overlapping tensors


def _model():
    ck = checkpoint.load(CKPT)
    return ck, mi.MfccInverter(config.from_checkpoint_hps(ck["hps"]))


def test_constructor_validation_param_groups_and_state_dict():
    ck, m = _model()
    for bad in (None, "yes", 2, 0.5, -1):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, 1e-3, track_update_ratio=bad)
    plain = optim.FusedAdam(m, 1e-3)
    assert plain.param_groups[0]["track_update_ratio"] is False      # off unless asked for
    opt = optim.FusedAdam(m, 1e-3, track_update_ratio=True)
    assert opt.param_groups[0]["track_update_ratio"] is True
    with pytest.raises(RuntimeError):                                # no engine yet: the error of the clip words
        opt.update_ratio
    with pytest.raises(RuntimeError):
        opt.grad_norm
    # flag off: the dictionary is what it was before the option existed
    sd_plain = plain.state_dict()
    assert set(sd_plain["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach",
                                                "capturable", "differentiable", "fused", "params"}
    # flag on: an extra key that torch.optim.Adam carries along, and the state stays in its format
    checkpoint.restore(m, opt, ck)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["track_update_ratio"] is True
    assert set(sd["param_groups"][0]) - {"track_update_ratio"} == set(sd_plain["param_groups"][0])
    params = [torch.nn.Parameter(torch.empty_like(p)) for p in m.parameters()]
    stock = torch.optim.Adam(params)
    stock.load_state_dict(sd)
    for i, p in enumerate(params):
        assert torch.equal(stock.state[p]["exp_avg"], ck["optim"]["state"][i]["exp_avg"])
    # round trip: a checkpoint with the key switches it on, one without it (torch.optim.Adam's own) leaves the constructor's
    opt2 = optim.FusedAdam(m, 1e-3)
    opt2.load_state_dict(ck["optim"])
    assert "track_update_ratio" not in ck["optim"]["param_groups"][0] and opt2.param_groups[0]["track_update_ratio"] is False
    opt2.load_state_dict(sd)
    assert opt2.param_groups[0]["track_update_ratio"] is True
    o2 = opt2.state_dict()
    assert o2["param_groups"][0] == sd["param_groups"][0]
    for i in sd["state"]:
        assert torch.equal(o2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(o2["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    # together with clipping: both extra keys
    both = optim.FusedAdam(m, 1e-3, max_grad_norm=2.0, track_update_ratio=True).state_dict()["param_groups"][0]
    assert both["max_grad_norm"] == 2.0 and both["track_update_ratio"] is True


# ----------------------------------------------------------------------------------------------
# two gloo ranks, both schedules, two tracked steps: the ratios against fp64 norms of each rank's own parameter copies
# ----------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ratio_worker(rank, world, port, bn, q, wg):
    from tests.test_dp_gloo import _global_batch, _seed_engine, _tiny
    from tests.update_ratio_emulator import emulate_uw
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny(bn)
        eng = emulate_uw(M.TrainEngine(hps, B=1, device="cpu", n_mel=5, wgrad_group=wg))
        d = dp.DataParallel()
        batch = _global_batch(eng.geom, 5, world)
        mine = [t[rank:rank + 1] for t in batch]
        gs = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
        n = eng.ps.numel
        names = eng.ps.names()
        out = {}
        for name in ("allreduce", "sharded"):
            _seed_engine(eng)
            eng.set_inputs(*mine)
            steps = []
            for it in range(2):
                before = eng.ps.params[:n].double().clone()
                if name == "allreduce":
                    d.train_step(eng, 1e-2, gs, track=True)
                else:
                    d.train_step_sharded(eng, 1e-2, gs, track=True)
                got = eng.update_ratios().clone().numpy()           # sharded: before the parameter all-gathers are waited for
                d.finish()
                after = eng.ps.params[:n].double()
                want = np.zeros((3, len(names)))
                for k, nm in enumerate(names):
                    o, ln = eng.ps.off[nm], eng.ps.numel_of(nm)
                    want[0, k] = float((before[o:o + ln] - after[o:o + ln]).norm())
                    want[1, k] = float(before[o:o + ln].norm())
                steps.append((got, want))
            out[name] = steps
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("bn,wg", [("ae", None), ("vqvae-ema", 1)])
def test_dp_tracked_steps_report_each_ranks_own_update_ratios(bn, wg):
    """Mean-type loss with two exchanged regions, and sum-type loss with three (wg = 1: the upper decoder layers' region
    has its own shard layout, so shard cuts fall inside tensors and chunks).  The sums are fp64 and the difference of two
    nearby fp32 values is exact, so the only errors are the fp32 roundings of the three outputs (6e-8 each): 1e-6."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ratio_worker, args=(r, world, port, bn, q, wg)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, o0), (_, o1) = res
    for name in ("allreduce", "sharded"):
        for it in range(2):
            (ga, wa), (gb, wb) = o0[name][it], o1[name][it]
            assert ga.tobytes() == gb.tobytes(), (name, it, "the ranks hold different ratios")
            checked = 0
            for got, want in ((ga, wa), (gb, wb)):
                assert (want[0] > 0).all(), "every tensor moved"
                for k in range(want.shape[1]):
                    assert abs(got[0, k] / want[0, k] - 1) < 1e-6, (name, it, k, got[0, k], want[0, k])
                    if want[1, k] > 0:
                        assert abs(got[1, k] / want[1, k] - 1) < 1e-6, (name, it, k, got[1, k], want[1, k])
                        assert abs(got[2, k] / (want[0, k] / want[1, k]) - 1) < 1e-6, (name, it, k, got[2, k])
                        checked += 1
                    else:
                        assert got[1, k] == 0.0 and np.isinf(got[2, k])
            assert checked > want.shape[1]                           # (more than half of the tensors have a weight norm)
