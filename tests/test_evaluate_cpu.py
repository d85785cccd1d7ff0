"""Held-out evaluation without a GPU: the numpy restatement of the accumulator (tests/eval_emulator.py) against plain
numpy; the evaluation plans of a TrainEngine built on 'cpu' (what they drop, where they write); those plans through the
CPU plan interpreter (same loss bits as the training forward, every protected buffer untouched); and the data-parallel
sum of the ranks' records over gloo."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, config, model as M
from tests import eval_emulator as EE
from tests.plan_emulator import Emu
from tests.test_plan_cpu import load, make_engine


# ----------------------------------------------------------------------------------------------
# the emulator against plain numpy
# ----------------------------------------------------------------------------------------------
def random_batch(rs, B, w, n_quant, Q, K, pitch=None, tgt_off=3):
    pitch = pitch or n_quant
    logits = rs.randn(B, w, pitch).astype(np.float32)
    wav = rs.randint(0, n_quant, (B, tgt_off + w + 5)).astype(np.float32)
    tgt = np.zeros((B, w), np.int64)
    tgt[:, :w - 1] = wav[:, tgt_off + 1: tgt_off + w].astype(np.int64)
    lg = logits[:, :, :n_quant].astype(np.float64)
    lsm = lg - np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True)) - lg.max(-1, keepdims=True)
    lp = np.take_along_axis(lsm, tgt[:, :, None], 2)[:, :, 0]
    live = np.ones((B, w)); live[:, w - 1] = 0
    nll = (-lp * live).astype(np.float32)
    ptgt = (np.exp(lp) * live).astype(np.float32)
    amax = np.argmax(logits[:, :, :n_quant], -1).astype(np.int32)          # (first maximum = lowest class)
    ind = rs.randint(0, K, Q).astype(np.int64) if Q else None
    dist = rs.rand(Q).astype(np.float32) if Q else None
    loss = rs.randn(5).astype(np.float32)
    return dict(nll=nll, ptgt=ptgt, wav=wav, tgt_off=tgt_off, amax=amax, logits=logits, n_quant=n_quant, ind=ind, dist=dist,
                loss=loss)


def plain_record(batches, K):
    """The record by np.sum in double (any order), counts as integers."""
    acc, hist = np.zeros(16), np.zeros(max(K, 1), np.int64)
    for b in batches:
        B, w = b["nll"].shape
        acc[0] += 1
        acc[1] += B * (w - 1)
        acc[2] += b["nll"][:, :w - 1].astype(np.float64).sum()
        acc[3] += b["ptgt"][:, :w - 1].astype(np.float64).sum()
        am = np.argmax(b["logits"][:, :w - 1, :b["n_quant"]], -1)           # (first maximum = lowest class)
        acc[4] += int((am == b["wav"][:, b["tgt_off"] + 1: b["tgt_off"] + w].astype(np.int64)).sum())
        if b["ind"] is not None:
            acc[5] += b["ind"].size
            acc[6] += b["dist"].astype(np.float64).sum()
            hist += np.bincount(b["ind"], minlength=K)
        acc[7:12] += b["loss"].astype(np.float64)
    return acc, hist


def entropy_bits(hist):
    """util.entropy as tests/plan_emulator.py restates it for the diagnostics op (util.py:98-105)."""
    h = torch.from_numpy(hist.astype(np.float64))
    n = h / h.sum()
    return float(-(n * torch.where(n == 0, torch.zeros_like(n), torch.log2(n))).sum())


@pytest.mark.parametrize("B,w,n_quant,Q,K", [(1, 2, 256, 1, 1), (1, 1025, 256, 7, 64), (3, 684, 256, 232, 4096),
                                             (2, 96, 16, 24, 64), (2, 40, 256, 0, 0)])
def test_emulator_against_plain_numpy(B, w, n_quant, Q, K):
    rs = np.random.RandomState(B * 1000 + w)
    batches = [random_batch(rs, B, w, n_quant, Q, K, pitch=64 if n_quant == 16 else None) for _ in range(3)]
    acc, hist = np.zeros(16), (np.zeros(K, np.uint32) if K else None)
    for i, b in enumerate(batches):
        kw = dict(b)
        if i == 1:                                       # the two arg-max forms count the same hits
            kw["amax"] = None
        EE.accumulate(acc, hist, **kw)
    want, whist = plain_record(batches, K)
    for i in (0, 1, 4, 5):                               # batches, positions, hits, queries: exact
        assert acc[i] == want[i], i
    if K:
        assert np.array_equal(hist.astype(np.int64), whist)
    for i in (2, 3, 6, 7, 8, 9, 10, 11):
        assert abs(acc[i] - want[i]) <= 1e-12 * max(abs(want[i]), 1e-300), (i, acc[i], want[i])
    assert not acc[12:].any()
    out = EE.finalize(acc, hist)
    n_pos = 3 * B * (w - 1)
    np.testing.assert_allclose(out[1], want[2] / n_pos, rtol=1e-6)
    np.testing.assert_allclose(out[2], want[2] / n_pos / np.log(2.0), rtol=1e-6)
    np.testing.assert_allclose(out[3], want[4] / n_pos, rtol=1e-6)
    np.testing.assert_allclose(out[4], want[3] / n_pos, rtol=1e-6)
    np.testing.assert_allclose(out[0], want[7] / 3, rtol=1e-6)
    np.testing.assert_allclose(out[9:13], want[8:12] / 3, rtol=1e-6)
    assert out[13] == n_pos and out[14] == 3 and out[15] == 0
    if K:
        ent = entropy_bits(whist)
        np.testing.assert_allclose(out[6], ent, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(out[7], 2.0 ** ent, rtol=1e-6)
        assert out[8] == (whist > 0).sum()
        np.testing.assert_allclose(out[5], want[6] / want[5], rtol=1e-6)
    else:
        assert not out[5:9].any()


def test_emulator_ties_take_the_lowest_class_and_an_empty_record_is_zero():
    lg = np.zeros((1, 3, 8), np.float32)
    lg[0, 0, [2, 5]] = 1.0                               # two classes tie: 2
    lg[0, 1, 7] = 3.0
    assert EE.argmax_lowest(lg).tolist() == [[2, 7, 0]]
    assert not EE.finalize(np.zeros(16), np.zeros(4, np.uint32)).any()


# ----------------------------------------------------------------------------------------------
# plan logic on a CPU engine
# ----------------------------------------------------------------------------------------------
class EvalEmu(Emu):
    """The plan interpreter with the evaluation accumulator (AEW_OP_EVAL_ACC) from tests/eval_emulator.py."""

    def op_30(self, p):
        acc_t, ao = self.flat(p.acc)
        acc = acc_t[ao:ao + 16].numpy()                              # (shares memory: updated in place)
        hist = None
        if p.hist:
            ht, ho = self.flat(p.hist)
            hist = ht[ho:ho + p.K].numpy().view(np.uint32)
        if p.finalize:
            self.wr(p.out, torch.arange(16), torch.from_numpy(EE.finalize(acc, hist)))
            return
        n = torch.arange(p.B * p.w)
        nll = self.rd(p.nll, n).numpy().reshape(p.B, p.w)
        ptgt = self.rd(p.ptgt, n).numpy().reshape(p.B, p.w)
        wav = self.rd(p.wav, torch.arange(p.B)[:, None] * p.wav_pitch + torch.arange(p.wav_pitch)[None, :]).numpy()
        kw = {}
        if p.amax:
            kw["amax"] = self.rd(p.amax, n).numpy().reshape(p.B, p.w)
        else:
            idx = (torch.arange(p.B)[:, None, None] * p.bs + torch.arange(p.w)[None, :, None] * p.pitch
                   + torch.arange(p.n_quant)[None, None, :])
            kw["logits"], kw["n_quant"] = self.rd(p.logits, idx).numpy(), p.n_quant
        if p.ind:
            kw["ind"] = self.rd(p.ind, torch.arange(p.Q)).numpy()
            kw["dist"] = self.rd(p.dist, torch.arange(p.Q)).numpy() if p.dist else None
        if p.loss:
            kw["loss"] = self.rd(p.loss, torch.arange(5)).numpy()
        EE.accumulate(acc, hist, nll, ptgt, wav, p.tgt_off, **kw)


def engines(golden_dir):
    """[(name, golden, engine, eps, tolerance check of the loss against the golden's reference loss)] - the engines
    tests/test_plan_cpu.py builds from the same fixtures, bf16 storage as on the device."""
    out = []
    z = load(golden_dir, "ae_tiny_vqvae-ema_random.npz")
    hps, eng = make_engine(z, "autoencoder", None)
    eng.emb.copy_(torch.from_numpy(z["emb0"]))
    eng.init_ema_from_emb()
    out.append(("vqvae-ema", z, eng, None, lambda v, z=z: abs(v / float(z["loss_intended"]) - 1) < 5e-3))
    z = load(golden_dir, "ae_tiny_vae_random.npz")
    hps, _ = make_engine(z, "autoencoder", None)
    hps2 = config.make_hps(**{**dict(hps), "bn_free_nats": float(z["free_nats"])})
    eng = M.TrainEngine(hps2, B=2, device="cpu", n_mel=9, take_compat=True)
    for k in eng.ps.names():
        eng.ps.view(k).copy_(torch.from_numpy(z["w." + k]))
    eng.set_anneal_weight(float(z["anneal"]))
    out.append(("vae", z, eng, torch.from_numpy(z["eps"]), lambda v, z=z: abs(v / float(z["loss"]) - 1) < 5e-3))
    z = load(golden_dir, "mi_tiny_identity.npz")
    hps, eng = make_engine(z, "mfcc_inverter", 7)
    out.append(("mi", z, eng, None, lambda v, z=z: abs(v - float(z["loss"])) < 2e-2))
    for _, _, eng, _, _ in out:
        assert eng.eval_acc is None and "eval.acc" not in eng.ws.bufs      # nothing until the first use ...
        eng.eval_plans()
        assert eng.eval_plans()[1] is eng.eval_b                            # ... and built once
    return out


def protected(eng):
    """{name: whole workspace buffer} of everything evaluate() must not write."""
    names = ["loss_buf", "met_buf", "diag", "diag_pk", "gstat", "adam_m", "adam_v"]
    if eng.bn_type == "vqvae-ema":
        names += ["emb", "ema_numer", "ema_denom", "ind_hist", "zn_sum", "n_sum_diag"]
    out = {"params": eng.ps.params, "grads": eng.ps.grads}
    for n in names:
        t = getattr(eng, n)
        out[n] = eng.ws.get(eng.ws.resolve(t.data_ptr())[0])
    if eng.adam_avg is not None:
        out["adam_avg"] = eng.adam_avg
    return out


def _recs(emu, tb):
    rt, roff = emu.flat(tb.recs)
    nb = tb.n_recs * C.sizeof(L.CopyRec)
    raw = bytes(rt[roff:roff + (nb + 7) // 8].numpy().tobytes())
    return (L.CopyRec * tb.n_recs).from_buffer_copy(raw[:nb])


# every address an op of an evaluation plan writes through, by op kind (a kind that is not listed fails the test)
OUTPUTS = {
    L.OP_GEMM_NT: lambda e, p: [p.out0.ptr, p.out1.ptr, p.out2.ptr, p.out3.ptr, p.counter, p.ksplit_ws, p.ksplit_tickets],
    L.OP_COPY_TABLE: lambda e, p: [r.dst for r in _recs(e, p)],
    L.OP_VQ_NEAREST: lambda e, p: [p.ind, p.dist, p.zq, p.scratch],
    L.OP_LC_GATHER: lambda e, p: [p.dst],
    L.OP_SPK_BIAS: lambda e, p: [p.bias, p.gc],
    L.OP_BASE_GATHER: lambda e, p: [p.x, p.onehot],
    L.OP_SOFTMAX_NLL: lambda e, p: [p.nll, p.ptgt, p.peak, p.amax] + ([p.dlogits] if p.backward else []),
    L.OP_REDUCE: lambda e, p: [p.out],
    L.OP_ZERO: lambda e, p: [p.ptr],
    L.OP_VAE: lambda e, p: [p.sample, p.kl_terms] + ([p.dlin] if p.backward else []),
    L.OP_AE_NORM: lambda e, p: [p.term] + ([p.dze] if p.backward else []),
    L.OP_NT_CHAIN: lambda e, p: [p.counters, p.sticky],
    L.OP_EVAL_ACC: lambda e, p: [p.acc, p.hist, p.out],
}


def test_evaluation_plans_drop_the_training_ops_and_write_no_protected_buffer(golden_dir):
    for name, z, eng, eps, _ in engines(golden_dir):
        emu = Emu(eng.ws)
        labs = eng.eval_a.labels + eng.eval_b.labels
        assert not set(labs) & set(M.TrainEngine.EVAL_DROP), name
        # ... and nothing else went missing: order preserved, the two new ops behind the softmax
        kept = [l for l in eng.fwd_a.labels + eng.fwd_b.labels if l not in M.TrainEngine.EVAL_DROP]
        assert labs == kept + ["eval.loss", "eval.accumulate"], name
        assert labs.index("eval.loss") > labs.index("softmax_nll")
        dropped = set(eng.fwd_a.labels + eng.fwd_b.labels) & set(M.TrainEngine.EVAL_DROP)
        assert {"metrics", "loss"} <= dropped and (name != "vqvae-ema" or {"vq.stats", "vq.ema", "diagnostics (codebook)"} <= dropped)
        for pl, src in ((eng.eval_a, eng.fwd_a), (eng.eval_b, eng.fwd_b)):
            lanes = {l: op.lane for l, op in zip(src.labels, src.ops)}
            assert all(op.lane == lanes[l] for l, op in zip(pl.labels, pl.ops) if l in lanes), name
        ranges = {k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in protected(eng).items()}
        for pl in (eng.eval_a, eng.eval_b, eng.eval_fin):
            for op, lab in zip(pl.array(), pl.labels):
                assert op.kind in OUTPUTS, (name, lab, op.kind)
                for ptr in OUTPUTS[op.kind](emu, getattr(op.u, L.OP_FIELD[op.kind])):
                    for k, (lo, hi) in ranges.items():
                        assert not (ptr and lo <= ptr < hi), (name, lab, k)
        ev = eng.eval_b.ops[-1].u.eva
        red, tr = eng.eval_b.ops[-2].u.red, eng.fwd_b.ops[eng.fwd_b.labels.index("loss")].u.red
        assert red.out == eng.eval_loss.data_ptr() and ev.loss == red.out and ev.acc == eng.eval_acc.data_ptr()
        plain = lambda v: list(v) if hasattr(v, "__len__") else v
        for f, _ in L.Reduce._fields_:                               # the same terms as the training loss
            assert f == "out" or plain(getattr(red, f)) == plain(getattr(tr, f)), (name, f)
        assert bool(ev.ind) == (name == "vqvae-ema") and bool(ev.amax) != bool(ev.logits)


def test_evaluation_plans_through_the_interpreter(golden_dir):
    for name, z, eng, eps, loss_ok in engines(golden_dir):
        eng.set_inputs(torch.from_numpy(z["wav"]), torch.from_numpy(z["mel"]), torch.from_numpy(z["voice"]),
                       torch.from_numpy(z["jitter"]), eps=eps)
        emu = EvalEmu(eng.ws)
        emu.run(eng.fwd_a)
        emu.run(eng.fwd_b)
        train_loss = eng.loss_buf[:5].numpy().copy()
        assert loss_ok(float(train_loss[0])), (name, train_loss[0])
        before = {k: t.numpy().tobytes() for k, t in protected(eng).items()}
        for n_eval in (1, 2):
            emu.run(eng.eval_a)
            emu.run(eng.eval_b)
            assert eng.eval_loss[:5].numpy().tobytes() == train_loss.tobytes(), name
            assert loss_ok(float(eng.eval_loss[0])), name
            for k, t in protected(eng).items():
                assert t.numpy().tobytes() == before[k], (name, k)
            acc = eng.eval_acc.numpy()
            B, w = eng.B, eng.n_win
            assert acc[0] == n_eval and acc[1] == n_eval * B * (w - 1)
            assert acc[7] == n_eval * np.float64(train_loss[0])
            if name == "vqvae-ema":
                assert acc[5] == n_eval * eng.Q
                want = n_eval * np.bincount(eng.ind[:eng.Q].numpy(), minlength=eng.K)
                assert np.array_equal(eng.eval_hist.numpy().view(np.uint32), want)
        emu.run(eng.eval_fin)
        out = eng.eval_out.numpy()
        n_pos = eng.B * (eng.n_win - 1)
        np.testing.assert_allclose(out[0], train_loss[0], rtol=1e-6)
        np.testing.assert_allclose(out[1], float(eng.dec.nll[:eng.B * eng.n_win].double().sum()) / n_pos, rtol=1e-6)
        np.testing.assert_allclose(out[4], float(eng.dec.ptgt[:eng.B * eng.n_win].double().sum()) / n_pos, rtol=1e-6)
        assert out[14] == 2 and out[13] == 2 * n_pos


# ----------------------------------------------------------------------------------------------
# data parallel: the ranks' records summed in one all-reduce (two gloo ranks)
# ----------------------------------------------------------------------------------------------
K_DP = 64


def _dp_batches():
    rs = np.random.RandomState(5)
    return [random_batch(rs, 2, 33, 256, 12, K_DP) for _ in range(4)]


def _record(batches):
    acc, hist = np.zeros(16), np.zeros(K_DP, np.uint32)
    for b in batches:
        EE.accumulate(acc, hist, **b)
    return acc, hist


def _dp_worker(rank, world, port, per_rank, q):
    import torch.distributed as dist
    from ae_wavenet_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d = dp.DataParallel()
        acc, hist = _record(_dp_batches()[rank * per_rank:(rank + 1) * per_rank])
        big = hist.copy()
        big[3] += np.uint32(0x90000000)                              # a count past 2^31: the int32 tensor holds unsigned words
        a_t, h_t = torch.from_numpy(acc.copy()), torch.from_numpy(big.view(np.int32).copy())
        s_acc, s_hist = d.sum_eval_record(a_t, h_t)
        assert s_hist.dtype == torch.int64
        assert a_t.numpy().tobytes() == acc.tobytes() and h_t.numpy().tobytes() == big.tobytes()       # arguments left alone
        h_t = torch.from_numpy(hist.view(np.int32).copy())
        # ... and through an engine (plans only, the interpreter in place of the device): the summed record is finalized
        # in the record's place and the rank's own comes back
        hps = config.make_hps("vqvae-ema", n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=3,
                              n_blocks=1, n_block_layers=2, enc_n_out=8, bn_n_out=4, bn_vq_n_embed=K_DP, n_win_batch=5)
        eng = M.TrainEngine(hps, B=1, device="cpu", n_mel=5)
        eng._run = lambda plan, timing=False: EvalEmu(eng.ws).run(plan)
        eng.eval_plans()
        eng.eval_acc.copy_(a_t)
        eng.eval_hist.copy_(h_t)
        out = d.eval_finish(eng).numpy().copy()
        assert eng.eval_acc.numpy().tobytes() == acc.tobytes() and eng.eval_hist.numpy().tobytes() == hist.tobytes()
        q.put((rank, s_acc.numpy().copy(), s_hist.numpy().copy(), out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("per_rank", [1, 2])
def test_dp_record_sum_two_gloo_ranks(per_rank):
    import torch.multiprocessing as mp
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, per_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    acc, hist = _record(_dp_batches()[:world * per_rank])            # the single-process record of all batches
    want_out = {r: EE.finalize(s_acc, hist) for r, s_acc, _, _ in res}          # (the summed acc of that rank, the true counts)
    hist = hist.astype(np.int64)
    codes = (hist > 0).sum()
    hist[3] += 2 * 0x90000000
    for r, s_acc, s_hist, out in res:                                # every rank holds the same sum
        assert out.tobytes() == want_out[r].tobytes() and out[14] == world * per_rank and out[8] == codes
        assert np.array_equal(s_hist, hist)
        for i in (0, 1, 4, 5):
            assert s_acc[i] == acc[i]
        if per_rank == 1:                                            # s1 + s2 is the same addition either way
            assert s_acc.tobytes() == acc.tobytes()
        else:
            assert np.all(np.abs(s_acc - acc) <= 1e-12 * np.abs(acc))
    assert res[0][1].tobytes() == res[1][1].tobytes()
