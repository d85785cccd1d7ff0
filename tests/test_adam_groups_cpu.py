"""Parameter groups of FusedAdam (per-tensor lr, decoupled weight decay, frozen tensors; aew_adam_groups_t) without a GPU:
the constructor and the pattern matching, requires_grad, a trajectory against torch.optim.AdamW, the other optimizer options
beside it, the state dictionaries and both data-parallel schedules on two gloo ranks - the plans executed by the CPU
interpreter of tests/adam_groups_emulator.py."""
import copy
import fnmatch
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import autoencoder_model as ae, checkpoint, config, dp, mfcc_inverter as mi, model as M, optim
from tests.accum_emulator import AccumEmu
from tests.adam_groups_emulator import GroupsEmu, emulate_groups
from tests.test_dp_gloo import _free_port, _global_batch, _seed_engine, _tiny

HERE = os.path.dirname(os.path.abspath(__file__))
CKPT = os.path.join(HERE, "golden", "reference_format.ckpt")
ADAM_GROUP_KEYS = {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
                   "fused", "params"}
# one frozen, one with another lr, one with decay (and the catch-all behind them: the bottleneck's projection)
THREE = [dict(params="encoder.*", frozen=True),
         dict(params="decoder.*.bias", lr=5e-3),
         dict(params="decoder.*", lr=2e-3, weight_decay=0.1)]
LR = 1e-2


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()


class _Emu(GroupsEmu):
    op_34 = AccumEmu.op_34                                         # (accumulate = 2 beside the groups)


def _surface(k=None, B=1):
    hps = _tiny("vqvae-ema")
    torch.manual_seed(5)
    model = ae.AutoEncoder(hps, n_mel=5, **({} if k is None else {"accumulate": k}))
    eng = emulate_groups(M.TrainEngine(hps, B=B, device="cpu", n_mel=5), _Emu)
    model._adopt_engine(eng)
    _seed_engine(eng)
    return model, eng


def _names(model):
    return [n for n, _ in model.named_parameters()]


def _grads(eng, steps, seed=40):
    """Flat gradients as a backward leaves them: random in the tensors, zero in the pad elements behind them."""
    n = eng.ps.numel
    mask = torch.zeros(n)
    for k in eng.ps.names():
        mask[eng.ps.off[k]:eng.ps.off[k] + eng.ps.numel_of(k)] = 1
    return [torch.randn(n, generator=torch.Generator().manual_seed(seed + i)) * 0.1 * mask for i in range(steps)]


# ----------------------------------------------------------------------------------------------
# 1. the constructor: rejected values, matching
# ----------------------------------------------------------------------------------------------
def test_constructor_rejects_what_the_issue_lists():
    m = ae.AutoEncoder(_tiny("vqvae-ema"), n_mel=5)
    ok = dict(params="decoder.*")
    for bad in (dict(ok, momentum=0.9), dict(ok, betas=(0.9, 0.99)), dict(lr=1e-3), "decoder.*", dict(params=[]), dict(params=3),
                dict(params="nothing.*"), dict(params=["decoder.*", "decoder.nope"]),
                dict(ok, lr=float("nan")), dict(ok, lr=float("inf")), dict(ok, lr=-1e-3), dict(ok, lr="x"), dict(ok, lr=None),
                dict(ok, weight_decay=float("nan")), dict(ok, weight_decay=float("inf")), dict(ok, weight_decay=-0.1),
                dict(ok, frozen=1), dict(ok, frozen="yes"), dict(ok, frozen=None), dict(ok, frozen=0.0)):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, LR, groups=[bad])
    for bad in (float("nan"), float("inf"), -1e-2, "x"):
        with pytest.raises(ValueError):
            optim.FusedAdam(m, LR, weight_decay=bad)
    with pytest.raises(ValueError):
        optim.FusedAdam(m, float("nan"), groups=[ok])
    opt = optim.FusedAdam(m, LR, groups=[dict(ok, lr=np.float32(0.5), weight_decay=torch.tensor(0.25), frozen=False)])
    assert opt.param_groups[0]["lr"] == 0.5 and opt.param_groups[0]["weight_decay"] == 0.25       # whatever float() takes
    # ... and what a schedule writes into a group is checked at the step
    m._engine = type("E", (), {"averaged_in": False, "avg_steps": 0})()
    for key, bad in (("lr", float("nan")), ("lr", -1.0), ("weight_decay", float("inf")), ("frozen", 1)):
        o = optim.FusedAdam(m, LR, groups=[dict(ok, weight_decay=0.1)])
        o.param_groups[0][key] = bad
        with pytest.raises(ValueError):
            o.step()
    m._engine = None


def test_matching_first_entry_wins_and_the_rest_is_a_last_group():
    m = ae.AutoEncoder(_tiny("vqvae-ema"), n_mel=5)
    names = _names(m)
    par = dict(m.named_parameters())
    opt = optim.FusedAdam(m, LR, weight_decay=0.3, groups=[
        dict(params=["encoder.*", "decoder.lc_conv.weight"], frozen=True),
        dict(params="decoder.*.bias", weight_decay=0.0),
        dict(params="decoder.*", lr=2e-5, weight_decay=1e-2)])
    want, taken = [], set()
    for pats in (["encoder.*", "decoder.lc_conv.weight"], ["decoder.*.bias"], ["decoder.*"]):     # by hand, with fnmatch
        mine = [n for n in names if n not in taken and any(fnmatch.fnmatchcase(n, p) for p in pats)]
        taken |= set(mine)
        want.append(mine)
    want.append([n for n in names if n not in taken])
    assert want[3] == ["bottleneck.linear.weight"]                     # the tensor no entry matches
    assert "decoder.lc_conv.bias" in want[1] and "decoder.lc_conv.weight" in want[0] and "decoder.post2.bias" in want[1]
    assert "decoder.post2.bias" not in want[2] and "decoder.post2.weight" in want[2]
    g = opt.param_groups
    assert len(g) == 4
    for k in range(4):
        assert [id(p) for p in g[k]["params"]] == [id(par[n]) for n in want[k]], k
        assert all(isinstance(p, torch.nn.Parameter) for p in g[k]["params"])
    assert (g[0]["lr"], g[0]["weight_decay"], g[0]["frozen"]) == (LR, 0.3, True)
    assert (g[1]["lr"], g[1]["weight_decay"], g[1]["frozen"]) == (LR, 0.0, False)
    assert (g[2]["lr"], g[2]["weight_decay"], g[2]["frozen"]) == (2e-5, 1e-2, False)
    assert (g[3]["lr"], g[3]["weight_decay"], g[3]["frozen"]) == (LR, 0.3, False)
    for k in range(4):                                                 # the optimizer-wide options are in every group's dict
        assert g[k]["betas"] == (0.9, 0.999) and g[k]["eps"] == 1e-8
    # an exact name is a pattern too; every tensor taken: no last group
    o2 = optim.FusedAdam(m, LR, groups=[dict(params="bottleneck.linear.weight", lr=1.0), dict(params="*")])
    assert [len(x["params"]) for x in o2.param_groups] == [1, len(names) - 1]
    # the records the step hands to the engine, in named_parameters() order
    rec = opt._tensor_records()
    assert len(rec) == len(names)
    for n, r in zip(names, rec):
        k = next(i for i in range(4) if n in want[i])
        assert r == (g[k]["lr"], g[k]["weight_decay"], g[k]["frozen"]), n
    # nothing a plain step does not do: no records, whatever the number of groups
    assert optim.FusedAdam(m, LR)._tensor_records() is None
    assert optim.FusedAdam(m, LR, groups=[dict(params="decoder.*"), dict(params="encoder.*", lr=LR)])._tensor_records() is None


# ----------------------------------------------------------------------------------------------
# 2. the step: requires_grad, a trajectory against torch.optim.AdamW
# ----------------------------------------------------------------------------------------------
def _run(model, eng, opt, grads, sched=None):
    n = eng.ps.numel
    for i, g in enumerate(grads):
        if sched is not None:
            sched(opt, i)
        eng.ps.grads[:n].copy_(g)
        opt.step()


def _spans(eng, names):
    return [(eng.ps.off[k], eng.ps.off[k] + eng.ps.numel_of(k)) for k in names]


def test_requires_grad_false_is_frozen_true():
    grads = None
    out = []
    for how in ("frozen", "requires_grad", "requires_grad, no groups", "nothing"):
        model, eng = _surface()
        n = eng.ps.numel
        grads = grads or _grads(eng, 2)
        start = eng.ps.params[:n].clone()
        if how == "frozen":
            opt = optim.FusedAdam(model, LR, groups=[dict(params="decoder.*", frozen=True)])
        elif how == "requires_grad":
            opt = optim.FusedAdam(model, LR, groups=[dict(params="decoder.*")])
        else:
            opt = optim.FusedAdam(model, LR)
        if how.startswith("requires_grad"):
            for k, p in model.named_parameters():
                if k.startswith("decoder."):
                    p.requires_grad_(False)
        _run(model, eng, opt, grads)
        out.append([bits(eng.ps.params[:n]), bits(eng.adam_m[:n]), bits(eng.adam_v[:n])])
        dec = [k for k in eng.ps.names() if k.startswith("decoder.")]
        for lo, hi in _spans(eng, dec):
            still = bits(eng.ps.params[lo:hi]) == bits(start[lo:hi])
            assert still == (how != "nothing"), (how, lo)
            if how != "nothing":
                assert not eng.adam_m[lo:hi].any() and not eng.adam_v[lo:hi].any()
        lo, hi = _spans(eng, ["encoder.net.0.conv.weight"])[0]
        assert bits(eng.ps.params[lo:hi]) != bits(start[lo:hi])
    assert out[0] == out[1] == out[2] != out[3]
    # ... and it is read at each step: unfrozen again, the tensor moves (with the global step count)
    model, eng = _surface()
    opt = optim.FusedAdam(model, LR)
    p = dict(model.named_parameters())["decoder.post1.weight"]
    (lo, hi), = _spans(eng, ["decoder.post1.weight"])
    p.requires_grad_(False)
    _run(model, eng, opt, grads[:1])
    kept = bits(eng.ps.params[lo:hi])
    p.requires_grad_(True)
    _run(model, eng, opt, grads[1:])
    assert bits(eng.ps.params[lo:hi]) != kept and eng.step_count == 2


def _sched(opt, i):
    """A per-group schedule that changes every trainable group's lr at every step."""
    opt.param_groups[1]["lr"] = 5e-4 * (0.5 ** i)
    opt.param_groups[2]["lr"] = 2e-4 / (1 + i)
    opt.param_groups[3]["lr"] = 1e-3 * (1 + 0.1 * i)


def test_five_steps_against_torch_adamw_with_the_same_groups():
    """tests/test_oracle_vs_golden.py::test_adam_matches_torch's figures for 5 steps (rtol 2e-6, atol 1e-7); the decay adds
    one fp32 rounding per step (6e-8 relative), well inside.  Like that test the rates stay at 1e-3 and below: the bound is
    an absolute one on the parameters, and the distance between ANY fp32 restatement of Adam and torch's grows with the
    rate (the step's relative rounding, some 1e-5 in its first steps, times lr)."""
    model, eng = _surface()
    n = eng.ps.numel
    names = eng.ps.names()
    assert names == _names(model)
    opt = optim.FusedAdam(model, 1e-3, ema_decay=0.9, groups=THREE)
    assert len(opt.param_groups) == 4
    start = eng.ps.params[:n].clone()
    ref = {k: torch.nn.Parameter(eng.ps.view(k).clone()) for k in names}
    idx = {id(p): i for i, (_, p) in enumerate(model.named_parameters())}
    stock = torch.optim.AdamW([dict(params=[ref[names[idx[id(p)]]] for p in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"])
                               for g in opt.param_groups[1:]], lr=1e-3)
    grads = _grads(eng, 5)
    for i, g in enumerate(grads):
        _sched(opt, i)
        for sg, og in zip(stock.param_groups, opt.param_groups[1:]):
            sg["lr"] = og["lr"]
        eng.ps.grads[:n].copy_(g)
        for k in names:
            ref[k].grad = eng.ps.view(k, grad=True).clone()
        opt.step()
        stock.step()
    frozen = [k for k in names if k.startswith("encoder.")]
    for k in names:
        if k in frozen:
            continue
        torch.testing.assert_close(eng.ps.view(k), ref[k].detach(), rtol=2e-6, atol=1e-7, msg=k)
        torch.testing.assert_close(eng.adam_m[eng.ps.off[k]:eng.ps.off[k] + eng.ps.numel_of(k)].view(ref[k].shape),
                                   stock.state[ref[k]]["exp_avg"], rtol=2e-6, atol=1e-7, msg=k)
        assert not torch.equal(eng.ps.view(k), start[eng.ps.off[k]:eng.ps.off[k] + eng.ps.numel_of(k)].view(ref[k].shape))
    # frozen tensors, their moments and their average: the bits they started with (the average starts from the parameters)
    for lo, hi in _spans(eng, frozen):
        hi = (hi + 3) // 4 * 4
        assert bits(eng.ps.params[lo:hi]) == bits(start[lo:hi]) == bits(eng.adam_avg[lo:hi])
        assert not eng.adam_m[lo:hi].any() and not eng.adam_v[lo:hi].any()
    assert eng.step_count == 5 and eng.avg_steps == 5


# ----------------------------------------------------------------------------------------------
# 3. beside the other options
# ----------------------------------------------------------------------------------------------
def test_clip_covers_the_trainable_tensors_and_more_than_eight_ranges_chain():
    model, eng = _surface()
    n = eng.ps.numel
    names = eng.ps.names()
    # every second tensor frozen: the trainable set has more than 8 element ranges, so the norm is a chain of launches
    opt = optim.FusedAdam(model, LR, max_grad_norm=0.05, groups=[dict(params="*.bias", frozen=True)])
    rec = opt._tensor_records()
    ranges = eng.trainable_ranges(rec)
    assert len(ranges) > 2 * L.GRAD_NORM_MAX_RANGES
    launches = []
    run = eng.clip.run
    eng.clip.run = lambda stream=0: (launches.append((eng.clip.array()[0].u.gnorm.n_ranges, eng.clip.array()[0].u.gnorm.finalize,
                                                      bool(eng.clip.array()[0].u.gnorm.add_in))), run(stream))[1]
    g = _grads(eng, 1)[0]
    eng.ps.grads[:n].copy_(g)
    for k, p in model.named_parameters():
        p.grad = eng.ps.view(k, grad=True).clone()
    trainable = [p for k, p in model.named_parameters() if not k.endswith(".bias")]
    want = float(torch.nn.utils.clip_grad_norm_(trainable, 0.05))
    before = eng.ps.params[:n].clone()
    opt.step()
    k8 = L.GRAD_NORM_MAX_RANGES
    assert len(launches) == (len(ranges) + k8 - 1) // k8 and sum(x[0] for x in launches) == len(ranges)
    assert [x[1] for x in launches] == [0] * (len(launches) - 1) + [1] and [x[2] for x in launches] == [False] + [True] * (len(launches) - 1)
    norm, coef = float(opt.grad_norm), float(opt.clip_coef)
    assert abs(norm / want - 1) < 1e-6 and coef < 1.0                    # fp64 sums against torch's fp32 norm
    assert coef == float(np.float32(0.05 / (np.sqrt(sum(float((g[lo:hi].double() ** 2).sum()) for lo, hi in ranges)) + 1e-6)))
    all_norm = float(g.double().norm())
    assert abs(norm / all_norm - 1) > 1e-3                               # ... not the norm over everything
    # the clipped gradient is what the trainable tensors' moments saw
    lo, hi = _spans(eng, ["decoder.post2.weight"])[0]
    torch.testing.assert_close(eng.adam_m[lo:hi], 0.1 * g[lo:hi] * coef, rtol=1e-6, atol=0)
    for lo, hi in _spans(eng, [k for k in names if k.endswith(".bias")]):
        assert bits(eng.ps.params[lo:hi]) == bits(before[lo:hi])
    # everything but one tensor frozen: the norm is that tensor's alone
    model, eng = _surface()
    opt = optim.FusedAdam(model, LR, max_grad_norm=1.0, groups=[dict(params="decoder.post1.weight"), dict(params="*", frozen=True)])
    eng.ps.grads[:n].copy_(g)
    opt.step()
    lo, hi = _spans(eng, ["decoder.post1.weight"])[0]
    assert abs(float(opt.grad_norm) / float(g[lo:hi].double().norm()) - 1) < 1e-6
    # nothing frozen: the one range of an optimizer without groups
    assert eng.trainable_ranges(None) == [(0, n)] == eng.trainable_ranges([(LR, 0.1, False)] * len(names))
    assert eng.trainable_ranges([(LR, 0.0, True)] * len(names)) == [(0, 0)]
    cut = eng.trainable_ranges(rec, [(n - 256, n), (0, 8)])              # cut to a caller's ranges, in the caller's order
    assert cut[-1] == (0, 8) and all(n - 256 <= lo < hi <= n for lo, hi in cut[:-1])
    assert sum(hi - lo for lo, hi in cut[:-1]) == sum(max(0, min(hi, n) - max(lo, n - 256)) for lo, hi in ranges)


def test_track_average_and_accumulate_beside_the_groups():
    # track_update_ratio: frozen rows read 0 / true norm / 0; the others the norms of what really happened
    model, eng = _surface()
    n = eng.ps.numel
    names = eng.ps.names()
    opt = optim.FusedAdam(model, LR, track_update_ratio=True, ema_decay=0.9, groups=THREE)
    g1, g2 = _grads(eng, 2)
    before = eng.ps.params[:n].double().clone()
    _run(model, eng, opt, [g1])
    after = eng.ps.params[:n].double()
    un, wn, ur = opt.update_norm, opt.weight_norm, opt.update_ratio
    for k, (lo, hi) in zip(names, _spans(eng, names)):
        w = float(before[lo:hi].norm())
        assert abs(float(wn[k]) / w - 1) < 1e-6, k
        if k.startswith("encoder."):
            assert float(un[k]) == 0.0 and float(ur[k]) == 0.0, k
        else:
            assert abs(float(un[k]) / float((before[lo:hi] - after[lo:hi]).norm()) - 1) < 1e-6, k     # p_old in front of the decay
            assert abs(float(ur[k]) / (float(un[k]) / w) - 1) < 1e-6, k
    # accumulate = 2: the mean scaling is unchanged - two micro-batches' sum with grad_scale / 2 is one step on the mean
    model2, eng2 = _surface(k=2)
    opt2 = optim.FusedAdam(model2, LR, track_update_ratio=True, ema_decay=0.9, groups=THREE)
    eng2.ps.grads[:n].copy_(g1 + g1)
    model2._group_ready = False
    opt2.step()                                                       # inside the group: nothing moves
    assert eng2.step_count == 0
    model2._group_ready = True
    opt2.step()
    assert eng2.step_count == 1 and model2.group_ready is False
    torch.testing.assert_close(eng2.ps.params[:n], eng.ps.params[:n], rtol=2e-6, atol=1e-7)
    lo, hi = _spans(eng, ["encoder.net.0.conv.weight"])[0]
    assert bits(eng2.ps.params[lo:hi]) == bits(before[lo:hi].float())
    # ema_decay: trainable tensors' average follows the recursion, frozen ones keep their bits
    from tests.weight_avg_emulator import avg_update
    want = avg_update(before.float().numpy(), optim.ema_rate_at(0.9, 0), eng.ps.params[:n].numpy())
    _run(model, eng, opt, [g2])
    want = avg_update(want, optim.ema_rate_at(0.9, 1), eng.ps.params[:n].numpy())
    assert bits(eng.adam_avg[:n]) == bits(want)
    assert bits(eng.adam_avg[lo:hi]) == bits(before[lo:hi].float())


# ----------------------------------------------------------------------------------------------
# 4. the table: uploaded when it changed, again after an engine rebuild
# ----------------------------------------------------------------------------------------------
def test_the_table_is_uploaded_only_when_a_value_changed():
    model, eng = _surface()
    n = eng.ps.numel
    opt = optim.FusedAdam(model, LR, groups=THREE)
    assert eng.adam_groups_tbl is None and "adam.groups" not in eng.ws.bufs       # allocated at first use
    g = _grads(eng, 1)[0]
    _run(model, eng, opt, [g])
    sent = eng._groups_sent
    P = len(eng.ps.names())
    assert sent == L.adam_tensor_records(opt._tensor_records(), P) and len(sent) == 16 * P == P * L.load().aew_sizeof(29)
    assert bits(eng.adam_groups_tbl[:4 * P]) == sent
    eng.adam_groups_tbl[:4 * P].zero_()                                 # an upload would repair this; none happens
    assert eng._groups_table(opt._tensor_records()) is None and not eng.adam_groups_tbl[:4 * P].any()
    opt.param_groups[2]["lr"] = 3e-3
    _run(model, eng, opt, [g])
    assert eng._groups_sent != sent and bits(eng.adam_groups_tbl[:4 * P]) == eng._groups_sent
    # the record: decay = fp32(1 - lr * weight_decay) computed in double
    rec = np.frombuffer(L.adam_tensor_records([(0.1, 0.3, False), (1e-4, 0.0, True)], 2), np.dtype("<f4,<f4,<i4,<i4"))
    assert rec[0][1] == np.float32(1.0 - 0.1 * 0.3) and rec[1][1] == np.float32(1.0) and (rec[0][2], rec[1][2]) == (0, 1)
    with pytest.raises(ValueError):
        L.adam_tensor_records([(0.1, 0.0, False)], 2)
    # a rebuilt engine starts without a table and gets it at its next step
    eng2 = emulate_groups(M.TrainEngine(_tiny("vqvae-ema"), B=2, device="cpu", n_mel=5))
    assert eng2._groups_sent is None and eng2.adam_groups_tbl is None
    lib = L.load()
    import ctypes as C
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(11) == C.sizeof(L.Adam) and lib.aew_sizeof(30) == C.sizeof(L.AdamGroups)
    assert lib.aew_sizeof(31) == C.sizeof(L.AdamGrouped) == C.sizeof(L.Adam) + 8 and L.OP_ADAM_GROUPS == L.OP_CODE_RUNS + 1
    assert L.OP_FIELD[L.OP_ADAM_GROUPS] == "adamg" and C.sizeof(L.Op) == lib.aew_sizeof(0)
    assert lib.aew_sizeof(29) == C.sizeof(L.AdamTensor) == 16


# ----------------------------------------------------------------------------------------------
# 5. state dictionaries
# ----------------------------------------------------------------------------------------------
def _ckpt_model():
    ck = checkpoint.load(CKPT)
    return ck, mi.MfccInverter(config.from_checkpoint_hps(ck["hps"]))


def test_state_dict_without_groups_is_the_dictionary_of_before():
    ck, m = _ckpt_model()
    plain = optim.FusedAdam(m, 1e-3)
    checkpoint.restore(m, plain, ck)
    sd = plain.state_dict()
    assert len(sd["param_groups"]) == 1 and set(sd["param_groups"][0]) == ADAM_GROUP_KEYS
    assert sd["param_groups"][0] == {
        "lr": plain.param_groups[0]["lr"], "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False,
        "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
        "params": list(range(len(list(m.parameters()))))}
    assert type(sd["param_groups"][0]["weight_decay"]) is int
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values()) and len(sd["state"]) == len(list(m.parameters()))
    # a frozen tensor by requires_grad is no option of the optimizer: still that dictionary
    next(iter(m.parameters())).requires_grad_(False)
    assert plain.state_dict()["param_groups"] == sd["param_groups"]


def test_state_dict_with_groups_loads_into_torch_adamw_and_round_trips():
    ck, m = _ckpt_model()
    names = _names(m)
    pats = [dict(params=names[0], frozen=True), dict(params="*.bias", weight_decay=0.0), dict(params="*", lr=2e-5, weight_decay=1e-2)]
    opt = optim.FusedAdam(m, 1e-3, max_grad_norm=2.0, groups=pats)
    opt.load_state_dict(ck["optim"])                                   # a one-group reference-format checkpoint: the moments load,
    assert [g["lr"] for g in opt.param_groups] == [1e-3, 1e-3, 2e-5]    # the per-group options keep the constructor's values
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.0, 1e-2] and opt.param_groups[0]["frozen"] is True
    sd = opt.state_dict()
    gs = sd["param_groups"]
    assert len(gs) == 3 and sorted(i for g in gs for i in g["params"]) == list(range(len(names)))
    assert gs[0]["params"] == [0] and gs[0]["frozen"] is True and "frozen" not in gs[1] and "frozen" not in gs[2]
    assert all(g["decoupled_weight_decay"] is True for g in gs) and gs[0]["max_grad_norm"] == 2.0 and "max_grad_norm" not in gs[1]
    assert [g["lr"] for g in gs] == [1e-3, 1e-3, 2e-5] and [g["weight_decay"] for g in gs] == [0.0, 0.0, 1e-2]
    assert all(ADAM_GROUP_KEYS <= set(g) for g in gs)
    for i, s in ck["optim"]["state"].items():
        assert torch.equal(sd["state"][i]["exp_avg"], s["exp_avg"]) and torch.equal(sd["state"][i]["exp_avg_sq"], s["exp_avg_sq"])
    # stock AdamW with the same grouping
    twins = [torch.nn.Parameter(torch.empty_like(p)) for p in m.parameters()]
    stock = torch.optim.AdamW([dict(params=[twins[i] for i in g["params"]]) for g in gs])
    stock.load_state_dict(copy.deepcopy(sd))
    assert [g["lr"] for g in stock.param_groups] == [1e-3, 1e-3, 2e-5] and stock.param_groups[2]["weight_decay"] == 1e-2
    for i, p in enumerate(twins):
        assert torch.equal(stock.state[p]["exp_avg"], ck["optim"]["state"][i]["exp_avg"]), i
    # round trip into a fresh optimizer with the same cut and other values: the file's per-group options come back
    _, m2 = _ckpt_model()
    opt2 = optim.FusedAdam(m2, 5e-1, groups=[dict(params=names[0]), dict(params="*.bias", lr=7.0), dict(params="*", weight_decay=0.5)])
    opt2.load_state_dict(sd)
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    assert opt2.param_groups[0]["frozen"] is True and opt2.param_groups[0]["max_grad_norm"] == 2.0
    for i in sd["state"]:
        assert torch.equal(sd2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
    # another cut: refused with the mismatch named, before anything is changed
    _, m3 = _ckpt_model()
    for other in ([dict(params="*.weight", lr=7.0)], [dict(params=names[1]), dict(params="*.bias"), dict(params="*")], None):
        opt3 = optim.FusedAdam(m3, 5e-1, **({} if other is None else {"groups": other}))
        was = copy.deepcopy([{k: v for k, v in g.items() if k != "params"} for g in opt3.param_groups])
        with pytest.raises(ValueError, match="group"):
            opt3.load_state_dict(sd)
        assert [{k: v for k, v in g.items() if k != "params"} for g in opt3.param_groups] == was and m3._opt_carry is None


# ----------------------------------------------------------------------------------------------
# 6. two gloo ranks, both schedules, three grouped steps with clipping == ONE process on the mean gradient
# ----------------------------------------------------------------------------------------------
def _dp_records(names):
    return [(1e-3, 0.0, True) if k.startswith("encoder.") else (5e-3, 0.0, False) if k.endswith(".bias") else (2e-3, 0.1, False)
            for k in names]


def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hps = _tiny("vqvae-ema")
        eng = emulate_groups(M.TrainEngine(hps, B=1, device="cpu", n_mel=5, wgrad_group=1))
        d = dp.DataParallel()
        batch = _global_batch(eng.geom, 5, world)
        gs = d.grad_scale(M.MEAN_LOSS[eng.bn_type])
        n = eng.ps.numel
        rec = _dp_records(eng.ps.names())
        out = {}
        for name in ("allreduce", "sharded"):
            _seed_engine(eng)
            eng.set_inputs(*[t[rank:rank + 1] for t in batch])
            start = eng.ps.params[:n].numpy().copy()
            coefs = []
            for it in range(3):
                step = d.train_step if name == "allreduce" else d.train_step_sharded
                step(eng, 1e-2, gs, max_grad_norm=0.5, track=True, groups=rec)
                d.finish()
                coefs.append(eng.grad_norm()[:2].numpy().copy())
            out[name] = (eng.ps.params[:n].numpy().copy(), coefs, start, eng.update_ratios().numpy().copy())
        ref = None
        if rank == 0:
            one = emulate_groups(M.TrainEngine(hps, B=world, device="cpu", n_mel=5))
            _seed_engine(one)
            one.set_inputs(*batch)
            rc = []
            for it in range(3):
                one.forward(); one.backward()
                one.adam_step(1e-2, 1.0, max_grad_norm=0.5, track=True, groups=rec)
                rc.append(one.grad_norm()[:2].numpy().copy())
            ref = (one.ps.params[:n].numpy().copy(), rc)
        q.put((rank, out, ref, [(eng.ps.off[k], eng.ps.off[k] + eng.ps.numel_of(k)) for k in eng.ps.names() if k.startswith("encoder.")]))
    finally:
        dist.destroy_process_group()


def test_both_dp_schedules_with_groups_match_one_process_on_the_mean_gradient():
    """wg = 1: three exchanged regions, so shard cuts fall inside tensors and chunks.  The parameters are bit-equal across
    the ranks and within 2e-5 of the largest weight of one process on the global batch - the bound tests/test_dp_gloo.py
    and tests/test_weight_avg_cpu.py hold that comparison to (the two runs' gradients differ in summation order)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref_p, ref_c = res[0][2]
    frozen = res[0][3]
    scale = float(np.abs(ref_p).max())
    for name in ("allreduce", "sharded"):
        (pa, ca, start, ra), (pb, cb, _, rb) = res[0][1][name], res[1][1][name]
        assert pa.tobytes() == pb.tobytes(), name
        assert ra.tobytes() == rb.tobytes(), name
        for it in range(3):
            assert ca[it].tobytes() == cb[it].tobytes(), (name, it)         # the clip coefficient: the same word on both ranks
            assert abs(ca[it][0] / ref_c[it][0] - 1) < 1e-5 and abs(ca[it][1] / ref_c[it][1] - 1) < 1e-5, (name, it, ca[it], ref_c[it])
            assert 0 < ca[it][1] < 1
        assert np.abs(pa - ref_p).max() <= 2e-5 * scale, (name, np.abs(pa - ref_p).max(), scale)
        for lo, hi in frozen:
            assert pa[lo:hi].tobytes() == start[lo:hi].tobytes(), (name, lo)
        assert not np.array_equal(pa, start)
