"""Gradient accumulation (AEW_OP_ACCUM, `accumulate=k`) without a GPU: the module surface, the engine methods and both
data-parallel schedules on CPU engines run by the interpreter of tests/accum_emulator.py.  The expectations are built from
the pieces that existed before the feature - a plain engine's forward / backward per micro-batch, its EMA plan and its
Adam step - and numpy fp32 additions in the documented order."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import autoencoder_model as ae, dp, mfcc_inverter as mi, model as M, optim
from tests.accum_emulator import ADD, FIRST, LAST, AccumEmu, emulate_accum, fold, sequential_sum
from tests.test_dp_gloo import _free_port, _global_batch, _seed_engine, _tiny
from tests.test_evaluate_cpu import EvalEmu

LR = 1e-2
MIN_USAGE = 0.005


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()


class _Emu(AccumEmu):
    op_30 = EvalEmu.op_30                                          # (evaluate() inside a group)


def _surface(k=1, B=1, **kw):
    hps = _tiny("vqvae-ema")
    torch.manual_seed(5)
    model = ae.AutoEncoder(hps, n_mel=5, **({} if k is None else {"accumulate": k}), **kw)
    eng = emulate_accum(M.TrainEngine(hps, B=B, device="cpu", n_mel=5), _Emu)
    model._adopt_engine(eng)
    _seed_engine(eng)
    return model, eng


def _plain(B=1):
    eng = emulate_accum(M.TrainEngine(_tiny("vqvae-ema"), B=B, device="cpu", n_mel=5))
    _seed_engine(eng)
    return eng


def _micro(eng, n, B=1, seed=3):
    batch = _global_batch(eng.geom, 5, n * B, seed=seed)
    return [[t[j * B:(j + 1) * B] for t in batch] for j in range(n)]


def _own(mb):
    """(gradient, z_sum | n_sum) of one micro-batch on a plain engine with the seeded weights and codebook."""
    eng = _plain(mb[0].shape[0])
    eng.set_inputs(*mb)
    eng.forward()
    eng.backward()
    return eng.ps.grads[:eng.ps.numel].numpy().copy(), eng.zn_sum.numpy().copy()


def _state(eng):
    n = eng.ps.numel
    out = [eng.ps.params[:n], eng.adam_m[:n], eng.adam_v[:n], eng.emb, eng.ema_numer, eng.ema_denom]
    if eng.adam_avg is not None:
        out.append(eng.adam_avg[:n])
    return [bits(t) for t in out] + [eng.step_count, eng.avg_steps]


# ----------------------------------------------------------------------------------------------
# 1. validation; k = 1 is the engine of today
# ----------------------------------------------------------------------------------------------
def test_validation_and_the_default_changes_nothing():
    hps = _tiny("vqvae-ema")
    for bad in (0, -1, True, False, 1.5, 2.0, "2", None, [2], np.float32(2)):
        with pytest.raises(ValueError, match="accumulate"):
            ae.AutoEncoder(hps, n_mel=5, accumulate=bad)
        with pytest.raises(ValueError, match="accumulate"):
            ae.AutoEncoder(hps, n_mel=5).set_accumulate(bad)
    with pytest.raises(ValueError, match="accumulate"):
        mi.MfccInverter(_tiny("vqvae-ema"), accumulate=0)
    assert ae.AutoEncoder(hps, n_mel=5).accumulate == 1 and ae.AutoEncoder(hps, n_mel=5, accumulate=np.int64(4)).accumulate == 4
    assert mi.MfccInverter(hps, accumulate=3).accumulate == 3
    one, eng1 = _surface(1)
    dflt, eng0 = _surface(None)
    mb = _micro(eng1, 1)[0]
    for model, eng in ((one, eng1), (dflt, eng0)):
        opt = optim.FusedAdam(model, lr=LR)
        for _ in range(2):
            opt.zero_grad()
            model.run(*mb)[2].backward()
            assert (model.micro_step, model.group_ready) == (0, False)
            opt.step()
        assert eng.acc_grads is None and eng.acc_stats is None and not eng.accum.ops
        assert "accum.grads" not in eng.ws.bufs and "accum.stats" not in eng.ws.bufs
    for name in ("fwd_a", "fwd_b", "bwd", "opt", "cb", "clip", "ratio"):
        a, b = getattr(eng1, name), getattr(eng0, name)
        assert a.labels == b.labels and [o.kind for o in a.ops] == [o.kind for o in b.ops], name
    assert list(eng1.ws.bufs) == list(eng0.ws.bufs) and _state(eng1) == _state(eng0) and eng1.step_count == 2
    assert L.OP_ACCUM == 34 and L.OP_FIELD[L.OP_ACCUM] == "accum" and (L.ACCUM_FIRST, L.ACCUM_ADD, L.ACCUM_LAST) == (0, 1, 2)


def test_emulator_fold_is_one_fp32_addition():
    a = np.array([1.0, 1e-8, 3.0, np.inf], np.float32)
    g = np.array([1e-8, 1.0, -3.0, -np.inf], np.float32)
    assert bits(fold(a, g, FIRST)[0]) == bits(g) and bits(fold(a, g, FIRST)[1]) == bits(g)
    acc, g2 = fold(a, g, ADD)
    assert bits(g2) == bits(g) and acc[:3].tolist() == [1.0, 1.0, 0.0] and np.isnan(acc[3])
    acc, g2 = fold(a, g, LAST)
    assert bits(acc) == bits(a) and g2[:3].tolist() == [1.0, 1.0, 0.0]
    x = [np.float32(1e8), np.float32(1.0), np.float32(-1e8)]
    assert sequential_sum([np.array([v]) for v in x])[0] == 0.0          # ((1e8 + 1) - 1e8) in fp32, in that order


# ----------------------------------------------------------------------------------------------
# 2. k = 3: gradients, statistics, one EMA, no-op steps, the step on the mean
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, dict(max_grad_norm=0.01, track_update_ratio=True, ema_decay=0.9)], ids=["plain", "clip+track+avg"])
def test_group_of_three(opts):
    _check_group_of_three(*_surface(3), opts)


def _check_group_of_three(model, eng, opts):
    n = eng.ps.numel
    opt = optim.FusedAdam(model, lr=LR, **opts)
    mbs = _micro(eng, 3, B=eng.B)
    own = [_own(mb) for mb in mbs]
    assert bits(own[0][0]) != bits(own[1][0]) != bits(own[2][0])
    g_sum, zn_sum = sequential_sum([o[0] for o in own]), sequential_sum([o[1] for o in own])
    cold = _state(eng)
    for j, mb in enumerate(mbs):
        assert (model.micro_step, model.group_ready) == (j, False)
        model.run(*mb)[2].backward()
        if j < 2:
            assert bits(eng.ps.grads[:n]) == bits(own[j][0])               # the micro-batch's own gradient
            assert bits(eng.zn_sum) == bits(own[j][1])
            for p_name, p in list(model.named_parameters())[:3]:
                assert bits(p.grad) == bits(eng.ps.view(p_name, grad=True))
            opt.step()                                                  # inside the group: nothing moves
            assert _state(eng) == cold and eng.adam_avg is None
    assert (model.micro_step, model.group_ready) == (0, True)
    assert bits(eng.ps.grads[:n]) == bits(g_sum)                        # ((g1 + g2) + g3), fp32
    assert bits(eng.zn_sum) == bits(zn_sum)
    assert bits(eng.acc_grads[:n]) == bits(sequential_sum([own[0][0], own[1][0]]))     # LAST leaves acc alone
    kd = eng.z_sum.numel()
    assert zn_sum[kd:].sum() == 3 * eng.Q and bits(zn_sum[kd:]) == bits(sum(o[1][kd:] for o in own))   # counts: exact
    # ONE EMA on the summed statistics (a plain engine's own EMA plan), then its codebook refresh - not three EMAs
    twin = _plain(eng.B)
    twin.zn_sum.copy_(torch.from_numpy(zn_sum))
    twin._run(twin.ema_plan)
    twin._run(twin.cb)
    assert bits(eng.ema_numer) == bits(twin.ema_numer) and bits(eng.ema_denom) == bits(twin.ema_denom)
    assert bits(eng.emb) == bits(twin.emb)
    thrice = _plain(eng.B)
    for o in own:
        thrice.zn_sum.copy_(torch.from_numpy(o[1]))
        thrice._run(thrice.ema_plan)
    assert bits(eng.ema_denom) != bits(thrice.ema_denom)
    # the step: a plain engine's Adam on the summed gradient with grad_scale / 3
    opt.step()
    assert model.group_ready is False and (eng.step_count, eng.avg_steps) == (1, 1 if opts else 0)
    twin.ps.grads[:n].copy_(torch.from_numpy(g_sum))
    kw = {}
    if opts:
        kw = dict(max_grad_norm=0.01, track=True, avg_rate=optim.ema_rate_at(0.9, 0))
    twin.adam_step(LR, 1.0 / 3, **kw)
    assert _state(eng) == _state(twin)
    if opts:
        assert bits(eng.clip_out[:4]) == bits(twin.clip_out[:4]) and float(eng.clip_out[1]) < 1.0
        assert bits(eng.update_ratios()) == bits(twin.update_ratios())
    opt.step()                                                          # consumed: a second step() is a no-op again
    assert eng.step_count == 1


# ----------------------------------------------------------------------------------------------
# 3. both loop idioms
# ----------------------------------------------------------------------------------------------
def test_harness_loop_and_torch_idiom_give_the_same_bits():
    k, out = 3, []
    for idiom in ("harness", "torch"):
        model, eng = _surface(k)
        opt = optim.FusedAdam(model, lr=LR)
        for i, mb in enumerate(_micro(eng, 2 * k)):
            if idiom == "harness":
                opt.zero_grad()                                         # chassis.py:157-160: every iteration
            model.run(*mb)[2].backward()
            opt.step()
            if idiom == "torch" and (i + 1) % k == 0:
                opt.zero_grad(set_to_none=False)
        assert eng.step_count == 2 and (model.micro_step, model.group_ready) == (0, False)
        out.append(_state(eng))
    assert out[0] == out[1]


# ----------------------------------------------------------------------------------------------
# 4. codebook upkeep happens once per group
# ----------------------------------------------------------------------------------------------
def test_restart_and_codebook_refresh_key_on_the_group():
    model, eng = _surface(3, codebook_restart=dict(every=2, min_usage=MIN_USAGE))
    opt = optim.FusedAdam(model, lr=LR)
    calls, ran = [], []
    inner, run = eng.restart_codes, eng._run
    eng.restart_codes = lambda *a, **kw: (calls.append((len(ran_bwd), a)), inner(*a, **kw))[1]
    eng._run = lambda plan, timing=False: (ran.append(plan.name), run(plan, timing))[1]
    ran_bwd = []
    for mb in _micro(eng, 6):
        model.run(*mb)[2].backward()
        ran_bwd.append(1)
        opt.step()
    assert calls == [(5, (MIN_USAGE, 2))]                               # once, inside backward number 6, call = 2
    assert ran.count(eng.cb.name) == 2 and ran.count("fwd_b") == 2 and ran.count("fwd_b_noema") == 4
    assert ran.count("bwd") == 6 and eng.step_count == 2
    # ... and without the every-step refresh no codebook plan runs at all
    model, eng = _surface(3, update_codebook_every_step=False)
    eng.update_codebook_every_step = False
    ran, run = [], eng._run
    eng._run = lambda plan, timing=False: (ran.append(plan.name), run(plan, timing))[1]
    for mb in _micro(eng, 3):
        model.run(*mb)[2].backward()
    assert ran.count(eng.cb.name) == 0 and ran.count("fwd_b") == 1


# ----------------------------------------------------------------------------------------------
# 5. refusals inside a group, reset, evaluate
# ----------------------------------------------------------------------------------------------
def test_mid_group_refusals_reset_and_evaluate():
    model, eng = _surface(3, B=2)
    mbs = _micro(eng, 3, B=2)
    model.set_accumulate(2)
    model.set_accumulate(3)                                             # between groups: fine
    model.run(*mbs[2])[2].backward()                                    # a micro-step of a group that will be discarded
    assert model.micro_step == 1
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.override(model.window_batch_size + 1)
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.run(*_micro(eng, 1, B=1)[0])                              # another batch size: another engine
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.sample(*[t[:1] for t in mbs[0]])                          # (the B = 1 engine)
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.set_accumulate(2)
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.to(torch.float64)
    assert model._engine is eng and (model.micro_step, model.accumulate) == (1, 3)
    n = eng.ps.numel
    held = bits(eng.acc_grads[:n]), bits(eng.acc_stats), bits(eng.ps.grads[:n]), bits(eng.zn_sum)
    before = _state(eng)
    model.evaluate(*mbs[1])                                             # allowed: writes neither gradients nor statistics
    assert (bits(eng.acc_grads[:n]), bits(eng.acc_stats), bits(eng.ps.grads[:n]), bits(eng.zn_sum)) == held
    assert _state(eng) == before and model.micro_step == 1
    # a run() whose backward never came has folded its statistics: the next run() says so instead of counting twice
    loss = model.run(*mbs[0])[2]
    with pytest.raises(L.AewError, match="reset_accumulation"):
        model.run(*mbs[1])
    del loss
    model.reset_accumulation()
    assert (model.micro_step, model.group_ready) == (0, False)
    model.override(model.window_batch_size)                             # (no change: no refusal either way)
    _seed_engine(eng)
    _check_group_of_three(model, eng, {})                               # the fresh group: the bits of test 2
    # an unstepped group is dropped by the next one, like an unstepped gradient
    for mb in mbs:
        model.run(*mb)[2].backward()
    assert (model.micro_step, model.group_ready) == (0, True)
    model.run(*mbs[0])[2].backward()
    assert (model.micro_step, model.group_ready) == (1, False)


def test_state_dict_keys_do_not_change():
    a, ea = _surface(3)
    b, eb = _surface(1)
    oa, ob = optim.FusedAdam(a, lr=LR, ema_decay=0.9), optim.FusedAdam(b, lr=LR, ema_decay=0.9)
    for mb in _micro(ea, 3):
        a.run(*mb)[2].backward()
        oa.step()
    b.run(*_micro(eb, 1)[0])[2].backward()
    ob.step()
    sa, sb = oa.state_dict(), ob.state_dict()
    assert set(sa) == set(sb) and set(sa["param_groups"][0]) == set(sb["param_groups"][0])
    assert set(sa["state"]) == set(sb["state"]) and all(set(sa["state"][i]) == set(sb["state"][i]) for i in sa["state"])
    assert list(a.state_dict()) == list(b.state_dict())
    # a checkpoint taken inside a group does not carry the group
    a.run(*_micro(ea, 1)[0])[2].backward()
    assert a.micro_step == 1 and list(a.state_dict()) == list(b.state_dict())
    assert set(oa.state_dict()["param_groups"][0]) == set(sb["param_groups"][0])


def test_engine_range_calls_follow_the_adam_rule():
    eng = _plain()
    n = eng.ps.numel
    g = torch.randn(n, generator=torch.Generator().manual_seed(1))
    eng.ps.grads[:n].copy_(g)
    eng.accum_grads(FIRST)
    lo = eng.dec_grad_offset
    eng.accum_grads(ADD, lo, n)
    eng.accum_grads(LAST, 0, lo)
    want = g.numpy().copy()
    assert bits(eng.acc_grads[:lo]) == bits(want[:lo]) and bits(eng.acc_grads[lo:n]) == bits(want[lo:] + want[lo:])
    assert bits(eng.ps.grads[:lo]) == bits(want[:lo] + want[:lo]) and bits(eng.ps.grads[lo:n]) == bits(want[lo:])
    assert len(eng.accum.ops) == 1 and eng.accum.ops[0].kind == L.OP_ACCUM
    for bad in ((2, n), (0, 6)):
        with pytest.raises(AssertionError):
            eng.accum_grads(ADD, *bad)
    with pytest.raises(ValueError):
        eng.accum_grads(3)
    none = emulate_accum(M.TrainEngine(_tiny("vae"), B=1, device="cpu", n_mel=5))
    with pytest.raises(L.AewError, match="vqvae-ema"):
        none.accum_stats(FIRST)


def test_launcher_refusals_come_before_any_launch():
    """Host memory, no stream: every refusal of aew_accum_t is returned before a HIP call, and nothing is written."""
    import ctypes as C
    lib = L.load()
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(25) == C.sizeof(L.Accum) == 32 and lib.aew_sizeof(24) == lib.aew_sizeof(26) == -1
    host = (C.c_uint8 * (16384 + 64))()
    a = (C.addressof(host) + 63) & ~63
    g, n = a + 8192, 1025

    def rc(acc, grd, n, mode):
        op = L.Op()
        op.kind = L.OP_ACCUM
        op.u.accum.acc, op.u.accum.g, op.u.accum.n, op.u.accum.mode = acc, grd, n, mode
        fail = C.c_int(-1)
        out = lib.aew_run_plan(C.byref(op), 1, None, C.byref(fail))
        assert out == 0 or fail.value == 0
        return out
    for args, want in [((a, g, -1, ADD), L.E_ARG), ((None, g, n, ADD), L.E_ARG), ((a, None, n, FIRST), L.E_ARG),
                       ((a, g, n, -1), L.E_ARG), ((a, g, n, 3), L.E_ARG), ((a, a, n, LAST), L.E_ARG),
                       ((a, a + 4096, n, ADD), L.E_ARG), ((a + 4096, a, n, ADD), L.E_ARG), ((a + 4, g, n, ADD), L.E_ALIGN),
                       ((a, g + 8, n, FIRST), L.E_ALIGN), ((None, None, 0, ADD), 0), ((a, g, 0, LAST), 0)]:
        assert rc(*args) == want, args
    assert bytes(host) == bytes(16384 + 64)


# ----------------------------------------------------------------------------------------------
# 6. two gloo ranks, both schedules, k = 2
# ----------------------------------------------------------------------------------------------
COUNTED = ("allreduce_grads", "_reduce_region", "allreduce_ema", "allreduce_ema_async")


def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = {}
        for sharded in (False, True):
            for k in (1, 2):
                model, eng = _surface(k)
                d = dp.DataParallel()
                d.attach(model, sharded=sharded)
                counts = {}
                for name in COUNTED:
                    def wrap(inner, name=name):
                        return lambda *a, **kw: (counts.__setitem__(name, counts.get(name, 0) + 1), inner(*a, **kw))[1]
                    setattr(d, name, wrap(getattr(d, name)))
                model._ema_allreduce = d.allreduce_ema_async if sharded else d.allreduce_ema
                own, cap, fold_in = [], {}, eng.accum_grads
                n = eng.ps.numel

                def spy(mode, lo=0, hi=None, cap=cap, eng=eng, fold_in=fold_in, n=n):
                    hi_ = n if hi is None else hi                       # what the backward wrote, before the fold
                    cap["cur"][lo:hi_] = eng.ps.grads[lo:hi_].numpy()
                    return fold_in(mode, lo, hi)
                eng.accum_grads = spy
                opt = optim.FusedAdam(model, lr=LR, grad_scale=d.grad_scale(M.MEAN_LOSS[eng.bn_type]))
                mbs = _micro(eng, world * k)[rank * k:(rank + 1) * k]
                per_micro = []
                for mb in mbs:
                    opt.zero_grad()
                    cap["cur"] = np.full(n, np.nan, np.float32)
                    model.run(*mb)[2].backward()
                    own.append(cap["cur"])
                    per_micro.append(dict(counts))
                    opt.step()
                d.finish()
                rec = dict(counts=dict(counts), per_micro=per_micro, params=bits(eng.ps.params[:n]), emb=bits(eng.emb),
                           numer=bits(eng.ema_numer), steps=eng.step_count)
                if k == 2:
                    assert np.array_equal(own[0], _own(mbs[0])[0]) and not np.isnan(own[1]).any()
                    mine = sequential_sum(own)
                    both = [torch.zeros(n) for _ in range(world)]
                    dist.all_gather(both, torch.from_numpy(mine))
                    total = (both[0].numpy() + both[1].numpy()).astype(np.float32)
                    got = eng.ps.grads[:n].numpy()
                    if not sharded:
                        rec["reduced_ok"] = got.tobytes() == total.tobytes()
                    else:                                               # this rank's shards and the replicated remainders
                        ok = True
                        for a, b in d._regions(eng):
                            s, rem = d._split(a, b)
                            for lo, hi in ((a + rank * s, a + (rank + 1) * s), (rem, b)):
                                ok = ok and got[lo:hi].tobytes() == total[lo:hi].tobytes()
                        rec["reduced_ok"] = ok
                    # a finished group nobody steps is dropped by the next one (sharded: its exchange is waited for first)
                    for mb in mbs:
                        cap["cur"] = np.zeros(n, np.float32)
                        model.run(*mb)[2].backward()
                    rec["ready"] = model.group_ready
                    for mb in mbs:
                        cap["cur"] = np.zeros(n, np.float32)
                        model.run(*mb)[2].backward()
                        opt.step()
                    d.finish()
                    rec["after_drop"] = (bits(eng.ps.params[:n]), bits(eng.emb), eng.step_count, d._st is None)
                out[(sharded, k)] = rec
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_data_parallel_exchanges_once_per_group():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for sharded in (False, True):
        for rank in range(world):
            step, group = res[rank][(sharded, 1)], res[rank][(sharded, 2)]
            assert step["counts"] and group["counts"] == step["counts"], (sharded, rank)     # per group == per step today
            assert group["per_micro"][0] == {}, "no collective inside the group"
            assert group["reduced_ok"] and group["steps"] == 1 and step["steps"] == 1
        for key in ("params", "emb", "numer", "after_drop"):
            assert res[0][(sharded, 2)][key] == res[1][(sharded, 2)][key], (sharded, key)
        assert res[0][(sharded, 2)]["ready"] and res[0][(sharded, 2)]["after_drop"][2:] == (2, True)
    assert res[0][(True, 2)]["after_drop"] == res[0][(False, 2)]["after_drop"]
    assert set(res[0][(False, 1)]["counts"]) == {"allreduce_grads", "allreduce_ema"}
    assert set(res[0][(True, 1)]["counts"]) == {"_reduce_region", "allreduce_ema_async"}
    assert res[0][(True, 2)]["params"] == res[0][(False, 2)]["params"]      # two ranks: a + b in either schedule
