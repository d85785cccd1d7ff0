"""Held-out evaluation on the GPU: AEW_OP_EVAL_ACC through ctypes -> C ABI against the numpy restatement of
tests/eval_emulator.py (record byte for byte, between canaries; finalize to the tolerance of the fused reductions), its
argument checks, and the module surface on the tiny models of tests/test_surface_gpu.py: evaluate() writes nothing a
training step reads, leaves a training trajectory bit-equal, accumulates what the emulator accumulates, follows the
averaged weights, refuses a stale backward and does not synchronise the host."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, config
from tests import eval_emulator as EE
from tests.test_evaluate_cpu import protected, random_batch
from tests.test_surface_gpu import _batch, _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
CANARY = {np.dtype(np.float32): -12345.5, np.dtype(np.float64): -54321.25, np.dtype(np.int32): -777, np.dtype(np.int64): -777}
TOL = 2e-5                       # tests/test_surface_gpu.py close(): the fused reductions' tolerance


def stream():
    return torch.cuda.current_stream().cuda_stream


def close(a, b, tol=TOL):
    a, b = float(a), float(b)
    assert abs(a - b) <= tol * max(1.0, abs(b)), (a, b)


class Case:
    """Every buffer of the op in an allocation of its own, PAD canary elements in front and behind."""

    def __init__(self, B, w, n_quant, Q, K, pitch, use_logits):
        self.B, self.w, self.n_quant, self.Q, self.K, self.pitch, self.use_logits = B, w, n_quant, Q, K, pitch, use_logits
        self.tgt_off = 3
        self.wav_pitch = self.tgt_off + w + 5
        sizes = dict(nll=(B * w, np.float32), ptgt=(B * w, np.float32), wav=(B * self.wav_pitch, np.float32),
                     amax=(B * w, np.int32), ind=(max(Q, 1), np.int64), dist=(max(Q, 1), np.float32), loss=(5, np.float32),
                     acc=(16, np.float64), hist=(max(K, 1), np.int32), out=(16, np.float32))
        if use_logits:
            sizes["logits"] = (B * w * pitch, np.float32)
        self.sizes = sizes
        self.dev = {}
        for k, (n, dt) in sizes.items():
            t = torch.from_numpy(np.full(n + 2 * PAD, CANARY[np.dtype(dt)], dt)).to(DEV)
            self.dev[k] = t
        self.view("acc").zero_()
        self.view("hist").zero_()
        self.view("out").fill_(7.0)

    def view(self, k):
        return self.dev[k][PAD:PAD + self.sizes[k][0]]

    def put(self, b):
        for k in ("nll", "ptgt", "wav", "amax", "loss") + (("logits",) if self.use_logits else ()) + (("ind", "dist") if self.Q else ()):
            self.view(k).copy_(torch.from_numpy(np.ascontiguousarray(b[k]).reshape(-1)))

    def op(self, finalize=False, codes=True, **over):
        op = L.Op()
        op.kind = L.OP_EVAL_ACC
        p = op.u.eva
        p.nll, p.ptgt, p.wav = (self.view(k).data_ptr() for k in ("nll", "ptgt", "wav"))
        p.wav_pitch, p.tgt_off, p.B, p.w = self.wav_pitch, self.tgt_off, self.B, self.w
        if self.use_logits:
            p.logits, p.bs, p.pitch, p.n_quant = self.view("logits").data_ptr(), self.w * self.pitch, self.pitch, self.n_quant
        else:
            p.amax = self.view("amax").data_ptr()
        if codes and self.Q:
            p.ind, p.dist, p.Q, p.K = self.view("ind").data_ptr(), self.view("dist").data_ptr(), self.Q, self.K
            p.hist = self.view("hist").data_ptr()
        p.loss, p.acc, p.out = self.view("loss").data_ptr(), self.view("acc").data_ptr(), self.view("out").data_ptr()
        p.finalize = int(finalize)
        for k, v in over.items():
            setattr(p, k, v)
        return op

    def launch(self, op):
        fail = C.c_int(-1)
        rc = L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
        torch.cuda.synchronize()
        return rc

    def got(self, keys=None):
        """{name: bytes of the whole allocation, canaries included}"""
        return {k: t.cpu().numpy().tobytes() for k, t in self.dev.items() if keys is None or k in keys}

    def framed(self, k, v):
        can = np.full(PAD, CANARY[v.dtype], v.dtype)
        return np.concatenate([can, v.reshape(-1), can]).tobytes()


def rolled(base, shift):
    """The batch with every per-position / per-query array rolled by `shift` (the targets stay: the op does not care
    whether nll and targets belong together)."""
    out = {}
    for k, v in base.items():
        if not isinstance(v, np.ndarray) or k == "wav":
            out[k] = v.copy() if isinstance(v, np.ndarray) else v
        else:
            out[k] = np.roll(v, shift, axis=1 if v.ndim >= 2 else 0).copy()
    return out


def special(b, i):
    """The inputs the op must get right whatever they hold."""
    B, w = b["nll"].shape
    o = b["tgt_off"]
    b["nll"][:, w - 1] = 1e30                            # position u = w - 1 is dropped, whatever sits there:
    b["ptgt"][:, w - 1] = -1e30
    b["amax"][:, w - 1] = b["wav"][:, o + w].astype(np.int32)       # it would count as a hit
    if w > 3:                                            # targets equal to and different from the arg-max, for certain
        b["wav"][:, o + 1] = b["amax"][:, 0]                                 # u = 0: a hit
        b["wav"][:, o + 2] = (b["amax"][:, 1] + 1) % b["n_quant"]           # u = 1: a miss
    if i == 1:
        b["ind"][:] = b["ind"][0]                        # every query on one code
    return b


SHAPES = [(1, 2, 256, 1, 1), (1, 1025, 256, 7, 64), (3, 684, 256, 232, 4096), (2, 96, 16, 24, 64), (8, 5000, 256, 232, 4096)]


@pytest.mark.parametrize("B,w,n_quant,Q,K", SHAPES)
def test_op_against_the_emulator_between_canaries(B, w, n_quant, Q, K):
    use_logits = n_quant != 256
    pitch = 64 if use_logits else n_quant
    c = Case(B, w, n_quant, Q, K, pitch, use_logits)
    rs = np.random.RandomState(w + K)
    base = random_batch(rs, B, w, n_quant, Q, K, pitch=pitch)
    if use_logits:                                       # a row whose two top logits tie: the lowest class counts
        base["logits"][0, 0, :n_quant] = 0.0
        base["logits"][0, 0, [3, 9]] = 2.5
        base["logits"][1, 5, [0, 15]] = 9.0
        base["amax"] = EE.argmax_lowest(base["logits"][:, :, :n_quant])
        assert base["amax"][0, 0] == 3 and base["amax"][1, 5] == 0
    acc, hist = np.zeros(16), np.zeros(K, np.uint32)
    still = None
    for i in range(3):
        b = special(rolled(base, 5 * i), i)              # (rolled along the positions: the arg-max moves with the logits)
        c.put(b)
        if still is None:
            still = c.got(("nll", "ptgt", "wav", "amax", "ind", "dist", "loss", "out", "logits"))
        with_ind = i != 2                                # the third batch comes without codes (ind == NULL)
        assert c.launch(c.op(codes=with_ind)) == 0
        kw = dict(b, amax=None) if use_logits else dict(b, logits=None)
        if not with_ind:
            kw["ind"] = kw["dist"] = None
        EE.accumulate(acc, hist, **kw)
        got = c.got(("acc", "hist", "out"))
        assert got["acc"] == c.framed("acc", acc), (i, np.frombuffer(got["acc"], np.float64)[PAD:PAD + 16], acc)
        assert got["hist"] == c.framed("hist", hist.view(np.int32)), i
        assert got["out"] == still["out"], "accumulation does not write out"
    assert acc[0] == 3 and acc[1] == 3 * B * (w - 1) and acc[5] == 2 * Q
    assert w <= 3 or 3 * B <= acc[4] <= 3 * B * (w - 2)            # the forced hit and the forced miss of every row
    inputs = c.got(("nll", "ptgt", "wav", "amax", "ind", "dist", "loss", "logits"))
    assert c.launch(c.op(finalize=True)) == 0
    after = c.got()
    assert all(after[k] == inputs[k] for k in inputs) and after["acc"] == c.framed("acc", acc) and \
        after["hist"] == c.framed("hist", hist.view(np.int32))
    out = np.frombuffer(after["out"], np.float32)
    assert (out[:PAD] == CANARY[np.dtype(np.float32)]).all() and (out[PAD + 16:] == CANARY[np.dtype(np.float32)]).all()
    out, want = out[PAD:PAD + 16], EE.finalize(acc, hist)
    for i, name in enumerate(EE.OUT_NAMES):
        print(name, out[i], want[i])
        if name in ("codes_used", "positions", "batches"):
            assert out[i] == want[i], name
        else:
            close(out[i], want[i])
    assert out[15] == 0
    # finalize without a histogram: the codebook entries are zero, the rest as before
    assert c.launch(c.op(finalize=True, codes=False)) == 0
    out2 = c.view("out").cpu().numpy()
    assert not out2[6:9].any() and out2[:6].tobytes() == out[:6].tobytes() and out2[9:].tobytes() == out[9:].tobytes()


def test_argument_errors_come_before_any_launch():
    c = Case(2, 96, 16, 24, 64, 64, True)
    c.put(random_batch(np.random.RandomState(0), 2, 96, 16, 24, 64, pitch=64))
    before = c.got()
    acc_p, nll_p, ind_p = c.view("acc").data_ptr(), c.view("nll").data_ptr(), c.view("ind").data_ptr()
    bad = [(dict(B=0), L.E_ARG), (dict(w=0), L.E_ARG), (dict(w=1), L.E_ARG), (dict(K=0), L.E_ARG), (dict(acc=None), L.E_ARG),
           (dict(nll=None), L.E_ARG), (dict(ptgt=None), L.E_ARG), (dict(logits=None), L.E_ARG), (dict(n_quant=0), L.E_ARG),
           (dict(hist=None), L.E_ARG), (dict(acc=acc_p + 4), L.E_ALIGN), (dict(nll=nll_p + 2), L.E_ALIGN),
           (dict(ptgt=nll_p + 1), L.E_ALIGN), (dict(ind=ind_p + 4), L.E_ALIGN), (dict(dist=nll_p + 3), L.E_ALIGN),
           (dict(loss=nll_p + 2), L.E_ALIGN), (dict(hist=nll_p + 1), L.E_ALIGN), (dict(logits=nll_p + 2), L.E_ALIGN)]
    for over, want in bad:
        assert c.launch(c.op(**over)) == want, over
    for over, want in [(dict(acc=None), L.E_ARG), (dict(out=None), L.E_ARG), (dict(K=0), L.E_ARG),
                       (dict(acc=acc_p + 4), L.E_ALIGN), (dict(out=nll_p + 2), L.E_ALIGN)]:
        assert c.launch(c.op(finalize=True, **over)) == want, over
    assert c.got() == before                             # canaries and contents: nothing ran


# ----------------------------------------------------------------------------------------------
# module surface
# ----------------------------------------------------------------------------------------------
def _mi():
    from ae_wavenet_amd import mfcc_inverter as mi
    hps = config.make_hps("mi", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, n_win_batch=96, n_blocks=2,
                          n_block_layers=3, n_global_embed=4, n_speakers=5)
    torch.manual_seed(3)
    m = mi.MfccInverter(hps).to(DEV)
    return hps, m


def _mi_batch(m, hps, B, seed):
    g = m.geom
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(DEV),
            torch.randn(B, hps.n_lc_in, g.mel_len, generator=gen).to(DEV),
            torch.randint(0, 5, (B,), generator=gen).to(DEV), torch.arange(g.embed_len).repeat(B, 1).to(DEV))


def _snapshot(m):
    eng = m._engine
    torch.cuda.synchronize()
    snap = {k: t.cpu().numpy().tobytes() for k, t in protected(eng).items()}
    snap.update({"metric." + k: (v.cpu().numpy().tobytes() if torch.is_tensor(v) else v) for k, v in m.objective.metrics.items()})
    snap["tprb_m"] = m.tprb_m.cpu().numpy().tobytes()
    snap["counters"] = (eng.step_count, eng.weights_version, eng.avg_steps)
    return snap


@pytest.mark.parametrize("kind", ["vqvae-ema", "vqvae", "vae", "ae", "mi"])
def test_evaluate_writes_nothing_a_training_step_reads(kind):
    if kind == "mi":
        hps, m = _mi()
        b0, b1 = _mi_batch(m, hps, 2, 2), _mi_batch(m, hps, 2, 4)
    else:
        hps, m = _tiny(kind, bn_n_out=16 if kind == "vae" else 8)
        b0, b1 = _batch(m, 2), _batch(m, 2, seed=4)
    kw = {}
    if kind == "vae":
        m.objective.update_anneal_weight(0.3)
        kw["eps"] = torch.randn(2, m.geom.embed_len, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    _, _, loss = m.run(*b0, **kw)
    loss.backward()                                      # (gradients, gradient statistics and the codebook refresh are in)
    before = _snapshot(m)
    l1 = m.evaluate(*b1, **kw)
    l2 = m.evaluate(*b1, **kw)
    assert l1.dim() == 0 and l1.device.type == "cuda" and not l1.requires_grad
    after = _snapshot(m)
    assert list(after) == list(before)
    for k in before:
        assert after[k] == before[k], k
    _, _, l3 = m.run(*b1, **kw)
    torch.cuda.synchronize()
    a, b, c = (x.detach().cpu().numpy().tobytes() for x in (l1, l2, l3))
    assert a == b == c, (float(l1), float(l2), float(l3))
    assert math.isfinite(float(l1)) and float(l1) > 0


def _trajectory(with_eval):
    from ae_wavenet_amd import optim
    hps, m = _tiny()
    opt = optim.FusedAdam(m, lr=1e-3, ema_decay=0.9, max_grad_norm=1.0)
    batch, other = _batch(m, 2), _batch(m, 2, seed=9)
    res = None
    for step in range(3):
        if with_eval:
            m.evaluate(*other)
        opt.zero_grad()
        _, _, loss = m.run(*batch)
        loss.backward()
        opt.step()
        if with_eval and step == 1:
            with opt.averaged_weights():
                with m.evaluation() as ev:
                    m.evaluate(*other)
                    m.evaluate(*batch)
                    res = {k: float(v) for k, v in ev.result().items()}
    torch.cuda.synchronize()
    eng = m._engine
    n = eng.ps.numel
    state = dict(params=eng.ps.params[:n], m=eng.adam_m[:n], v=eng.adam_v[:n], avg=eng.adam_avg[:n], emb=eng.emb,
                 ema_numer=eng.ema_numer, ema_denom=eng.ema_denom, ind_hist=eng.ind_hist)
    return {k: v.cpu().numpy().tobytes() for k, v in state.items()}, (eng.step_count, eng.avg_steps), res


def test_training_trajectory_is_bit_equal_with_evaluation_in_between():
    plain, cnt_a, _ = _trajectory(False)
    mixed, cnt_b, res = _trajectory(True)
    assert cnt_a == cnt_b == (3, 3)
    for k in plain:
        assert plain[k] == mixed[k], k
    assert res["batches"] == 2 and res["positions"] == 2 * 2 * 95 and math.isfinite(res["loss"]) and res["codes_used"] >= 1


def _engine_batch(eng):
    """What the engine's last forward left, as the emulator's arguments."""
    B, w = eng.B, eng.n_win
    sm = next(op.u.sm for op, lab in zip(eng.fwd_b.ops, eng.fwd_b.labels) if lab == "softmax_nll")
    b = dict(nll=eng.dec.nll[:B * w].view(B, w).cpu().numpy(), ptgt=eng.dec.ptgt[:B * w].view(B, w).cpu().numpy(),
             wav=eng.in_wav.cpu().numpy(), tgt_off=sm.tgt_off, loss=eng.eval_loss[:5].cpu().numpy())
    assert sm.wav_pitch == b["wav"].shape[1]
    if getattr(eng, "amax_buf", None) is not None:
        b["amax"] = eng.amax_buf[:B * w].view(B, w).cpu().numpy()
    else:
        b["logits"], b["n_quant"] = eng.logits().cpu().numpy(), eng.hps.n_quant
    b["ind"], b["dist"] = eng.ind[:eng.Q].cpu().numpy(), eng.min_dist[:eng.Q].cpu().numpy()
    return b


def test_evaluation_block_over_three_batches_of_two_sizes():
    hps, m = _tiny()
    K = hps.bn_vq_n_embed
    acc, hist = np.zeros(16), np.zeros(K, np.uint32)
    m.evaluate(*_batch(m, 2, seed=8))                    # outside a block: accumulates into a record nobody reads ...
    with m.evaluation() as ev:                           # ... which the block starts from zero
        for B, seed in ((2, 1), (2, 2), (1, 3)):
            m.evaluate(*_batch(m, B, seed=seed))
            torch.cuda.synchronize()
            EE.accumulate(acc, hist, **_engine_batch(m._engine))
        res = {k: v for k, v in ev.result().items()}
        assert all(v.dim() == 0 and v.device.type == "cuda" for v in res.values()) and list(res) == list(EE.OUT_NAMES)
        res = {k: float(v) for k, v in res.items()}
    eng = m._engine
    assert eng.B == 1 and eng.eval_acc.cpu().numpy().tobytes() == acc.tobytes(), "the record moved with the model, bit for bit"
    assert eng.eval_hist.cpu().numpy().tobytes() == hist.tobytes()
    want = EE.finalize(acc, hist)
    for i, name in enumerate(EE.OUT_NAMES):
        print(name, res[name], want[i])
        if name in ("codes_used", "positions", "batches"):
            assert res[name] == want[i], name
        else:
            close(res[name], want[i])
    assert res["batches"] == 3 and res["positions"] == 5 * 95
    # bits_per_sample * ln 2 == nll to one fp32 ulp: out[1] and out[2] are ONE double value n, rounded to fp32 as n and as
    # n / ln 2, so each is off by at most half an ulp of itself; on the nll's scale that is 0.5 * ln 2 ulp(bits) + 0.5 ulp(nll)
    # <= (0.35 + 0.5) ulp(bits), the ulp of the larger number (ulp(nll) <= ulp(bits))
    bits, nll = np.float32(res["bits_per_sample"]), np.float32(res["nll"])
    assert abs(float(bits) * math.log(2.0) - float(nll)) <= float(np.spacing(bits))


def test_evaluate_inside_averaged_weights_is_a_fresh_model_with_those_weights():
    from ae_wavenet_amd import optim
    hps, m = _tiny()
    opt = optim.FusedAdam(m, lr=1e-2, ema_decay=0.5, ema_warmup=False)
    batch, held = _batch(m, 2), [_batch(m, 2, seed=6), _batch(m, 2, seed=7)]
    for _ in range(2):
        opt.zero_grad()
        _, _, loss = m.run(*batch)
        loss.backward()
        opt.step()
    with m.evaluation() as ev:
        for h in held:
            m.evaluate(*h)
        raw = {k: float(v) for k, v in ev.result().items()}
    with opt.averaged_weights():
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        with m.evaluation() as ev:
            losses = [m.evaluate(*h) for h in held]
            avg = {k: v.cpu().numpy().tobytes() for k, v in ev.result().items()}
    hps2, fresh = _tiny()
    fresh.load_state_dict(sd)
    with fresh.evaluation() as ev:
        losses2 = [fresh.evaluate(*h) for h in held]
        got = {k: v.cpu().numpy().tobytes() for k, v in ev.result().items()}
    assert got == avg
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(losses, losses2))
    assert raw["nll"] != float(np.frombuffer(avg["nll"], np.float32)[0]), "the averaged weights are other weights"


def test_backward_after_evaluate_raises_and_writes_no_gradient():
    hps, m = _tiny()
    a, b = _batch(m, 2), _batch(m, 2, seed=4)
    _, _, loss = m.run(*a)
    loss.backward()
    torch.cuda.synchronize()
    eng = m._engine
    grads = eng.ps.grads.cpu().numpy().tobytes()
    gmul = eng.gmul.cpu().numpy().tobytes()
    _, _, loss = m.run(*b)
    m.evaluate(*a)
    with pytest.raises(L.AewError, match="evaluate"):
        (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert eng.ps.grads.cpu().numpy().tobytes() == grads and eng.gmul.cpu().numpy().tobytes() == gmul
    _, _, loss = m.run(*b)                               # and the next step is an ordinary one
    loss.backward()
    torch.cuda.synchronize()
    assert eng.ps.grads.cpu().numpy().tobytes() != grads
    # another batch size in between: the loss belongs to an engine that is no longer the live one
    _, _, loss = m.run(*b)
    m.evaluate(*_batch(m, 1, seed=5))
    with pytest.raises(L.AewError, match="evaluate"):
        loss.backward()


def test_evaluate_does_not_synchronise_the_host():
    hps, m = _tiny()
    batch = _batch(m, 2)
    m.evaluate(*batch)                                   # builds the engine, captures the plans
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")              # .item() / .cpu() / a blocking copy would raise
    try:
        with m.evaluation() as ev:
            loss = m.evaluate(*batch)
            loss2 = m.evaluate(*batch)
            res = ev.result()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(loss) == float(loss2) and float(res["batches"]) == 2
