"""Evaluation by group on the GPU: AEW_OP_EVAL_GROUPS through ctypes -> C ABI against the numpy restatement of
tests/eval_groups_emulator.py (the record byte for byte, between canaries; finalize exact in its counts, to one fp32
rounding in its means and to the margin of the device's log2 in its entropies), its argument checks, and the module
surface on the tiny models of tests/test_surface_gpu.py: grouping leaves Evaluator.result() and a training trajectory
bit-equal, splits what the plain record holds, does not synchronise the host, and agrees with codes.voice_information."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, codes as CD
from tests import eval_emulator as EE
from tests import eval_groups_emulator as EG
from tests.test_evaluate_cpu import random_batch
from tests.test_evaluate_gpu import CANARY, PAD, TOL, _mi, _mi_batch, rolled, special, stream
from tests.test_surface_gpu import _batch, _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT_G, MEAN_G, LOG_G = (0, 1, 7, 10, 11), (2, 3, 4, 5, 6), (8, 9)
EXACT_T, LOG_T = (0, 8, 9, 10, 11, 12, 13, 14, 15), (1, 2, 3, 4, 5, 6, 7)


class Case:
    """Every buffer of the op in an allocation of its own, PAD canary elements in front and behind."""

    def __init__(self, B, w, Qw, K, G, n_quant=256, pitch=256, use_logits=False, codes_only=False):
        self.B, self.w, self.Qw, self.K, self.G = B, w, Qw, K, G
        self.n_quant, self.pitch, self.use_logits, self.codes_only = n_quant, pitch, use_logits, codes_only
        self.tgt_off = 3
        self.wav_pitch = self.tgt_off + w + 5
        sizes = dict(ind=(B * Qw, np.int64), dist=(B * Qw, np.float32), group=(B, np.int64), gacc=(G * 8, np.float64),
                     ghist=(G * K, np.int32), gtot=(4, np.float64), win=(B * 4, np.float64), gout=(G * 12, np.float32),
                     tout=(16, np.float32), scratch=(K + 4 * G, np.float64))
        if not codes_only:
            sizes.update(nll=(B * w, np.float32), ptgt=(B * w, np.float32), wav=(B * self.wav_pitch, np.float32),
                         amax=(B * w, np.int32))
            if use_logits:
                sizes["logits"] = (B * w * pitch, np.float32)
        self.sizes = sizes
        self.dev = {k: torch.from_numpy(np.full(n + 2 * PAD, CANARY[np.dtype(dt)], dt)).to(DEV) for k, (n, dt) in sizes.items()}
        self.zero()
        self.view("gout").fill_(7.0)
        self.view("tout").fill_(7.0)

    def zero(self):
        for k in ("gacc", "ghist", "gtot", "win"):
            self.view(k).zero_()

    def view(self, k):
        return self.dev[k][PAD:PAD + self.sizes[k][0]]

    def put(self, b, group):
        keys = ("ind", "dist") if self.codes_only else ("nll", "ptgt", "wav", "amax", "ind", "dist") + (("logits",) if self.use_logits else ())
        for k in keys:
            self.view(k).copy_(torch.from_numpy(np.ascontiguousarray(b[k]).reshape(-1)))
        self.view("group").copy_(torch.from_numpy(np.asarray(group, np.int64)))

    def op(self, finalize=False, codes=True, **over):
        op = L.Op()
        op.kind = L.OP_EVAL_GROUPS
        p = op.u.evg
        p.B, p.w, p.G = self.B, self.w, self.G
        if not self.codes_only:
            p.nll, p.ptgt, p.wav = (self.view(k).data_ptr() for k in ("nll", "ptgt", "wav"))
            p.wav_pitch, p.tgt_off = self.wav_pitch, self.tgt_off
            if self.use_logits:
                p.logits, p.bs, p.pitch, p.n_quant = self.view("logits").data_ptr(), self.w * self.pitch, self.pitch, self.n_quant
            else:
                p.amax = self.view("amax").data_ptr()
        if codes:
            p.ind, p.dist, p.Qw, p.K = self.view("ind").data_ptr(), self.view("dist").data_ptr(), self.Qw, self.K
            p.ghist, p.scratch = self.view("ghist").data_ptr(), self.view("scratch").data_ptr()
        p.group = self.view("group").data_ptr()
        p.gacc, p.gtot, p.win = (self.view(k).data_ptr() for k in ("gacc", "gtot", "win"))
        p.gout, p.tout = self.view("gout").data_ptr(), self.view("tout").data_ptr()
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
        return {k: t.cpu().numpy().tobytes() for k, t in self.dev.items() if keys is None or k in keys}

    def framed(self, k, v):
        v = np.ascontiguousarray(v)
        can = np.full(PAD, CANARY[v.dtype], v.dtype)
        return np.concatenate([can, v.reshape(-1), can]).tobytes()

    def inner(self, blob, k):
        n, dt = self.sizes[k]
        a = np.frombuffer(blob, dt)
        assert (a[:PAD] == CANARY[np.dtype(dt)]).all() and (a[PAD + n:] == CANARY[np.dtype(dt)]).all(), k
        return a[PAD:PAD + n]


def check_finalize(c, rec):
    """One finalize launch against the emulator; returns (gout, tout) as the device wrote them."""
    gacc, ghist, gtot, _ = rec
    before = c.got([k for k in c.dev if k not in ("gout", "tout", "scratch")])
    assert c.launch(c.op(finalize=True)) == 0
    after = c.got()
    assert all(after[k] == before[k] for k in before), "finalize writes gout / tout / scratch only"
    c.inner(after["scratch"], "scratch")
    gout, tout = c.inner(after["gout"], "gout").reshape(c.G, 12), c.inner(after["tout"], "tout")
    w_gout, w_tout = EG.finalize(gacc, ghist, gtot)
    for g in range(c.G):
        for i in EXACT_G:
            assert gout[g, i] == w_gout[g, i], (g, i, gout[g, i], w_gout[g, i])
        for i in MEAN_G:
            assert abs(float(gout[g, i]) - float(w_gout[g, i])) <= 1e-6 * abs(float(w_gout[g, i])), (g, i, gout[g, i], w_gout[g, i])
        for i in LOG_G:
            assert abs(float(gout[g, i]) - float(w_gout[g, i])) <= TOL * max(1.0, abs(float(w_gout[g, i]))), (g, i, gout[g, i], w_gout[g, i])
    for i in EXACT_T:
        assert tout[i] == w_tout[i], (i, tout[i], w_tout[i])
    for i in LOG_T:
        print(EG.TOUT_NAMES[i], tout[i], w_tout[i])
        assert abs(float(tout[i]) - float(w_tout[i])) <= TOL * max(1.0, abs(float(w_tout[i]))), (i, tout[i], w_tout[i])
    return gout.copy(), tout.copy()


SHAPES = [(1, 2, 1, 1, 1, False), (3, 1030, 5, 70, 5, False), (3, 1030, 5, 70, 5, True), (8, 5000, 29, 4096, 40, False)]


@pytest.mark.parametrize("B,w,Qw,K,G,use_logits", SHAPES)
def test_op_against_the_emulator_between_canaries(B, w, Qw, K, G, use_logits):
    n_quant, pitch = (16, 64) if use_logits else (256, 256)
    c = Case(B, w, Qw, K, G, n_quant, pitch, use_logits)
    rs = np.random.RandomState(w + K)
    base = random_batch(rs, B, w, n_quant, B * Qw, K, pitch=pitch)
    if use_logits:                                       # rows whose two top logits tie exactly: the lowest class counts
        base["logits"][0, 0, :n_quant] = 0.0
        base["logits"][0, 0, [3, 9]] = 2.5
        base["logits"][1, 5, [0, 15]] = 9.0
        base["amax"] = EE.argmax_lowest(base["logits"][:, :, :n_quant])
        assert base["amax"][0, 0] == 3 and base["amax"][1, 5] == 0
    if B == 3:                                           # two windows share a group (the fold order matters), group 1 and 3 stay empty
        groups = [[2, 2, 0], [G, 2, -1], [4, 0, 2]]
    else:
        groups = [rs.randint(0, G, B) for _ in range(3)]
    runs = []
    for rep in range(2):                                 # twice from zero: bit-equal records and outputs
        c.zero()
        rec = EG.new_record(G, K, B)
        for i in range(3):
            b = special(rolled(base, 5 * i), i)
            if B == 3 and i == 1:                        # a code K and a code -1: counted nowhere
                b["ind"] = b["ind"].copy()
                b["ind"][Qw + 1], b["ind"][Qw + 3] = K, -1
            c.put(b, groups[i])
            assert c.launch(c.op()) == 0
            kw = {k: b[k] for k in ("nll", "ptgt", "wav", "tgt_off", "ind", "dist")}
            kw.update(dict(logits=b["logits"], n_quant=n_quant) if use_logits else dict(amax=b["amax"]))
            EG.accumulate(*rec, np.asarray(groups[i], np.int64), **kw)
            got = c.got(("gacc", "ghist", "gtot", "win", "gout", "tout"))
            assert got["gacc"] == c.framed("gacc", rec[0]), (i, c.inner(got["gacc"], "gacc").reshape(G, 8), rec[0])
            assert got["ghist"] == c.framed("ghist", rec[1].view(np.int32)), i
            assert got["gtot"] == c.framed("gtot", rec[2]) and got["win"] == c.framed("win", rec[3]), i
            if rep == 0:
                assert not (c.inner(got["gout"], "gout") != 7.0).any() and not (c.inner(got["tout"], "tout") != 7.0).any()
        if B == 3:
            assert rec[2].tolist() == [2, 3, 0, 0] and rec[0][:, 0].tolist() == [2, 0, 4, 0, 1] and rec[1].sum() == 7 * Qw - 2
        runs.append(check_finalize(c, rec))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    # without the table: the code entries are zero, tout holds the dropped windows and the batches alone
    assert c.launch(c.op(finalize=True, ghist=None, scratch=None)) == 0
    gout, tout = c.view("gout").cpu().numpy().reshape(G, 12), c.view("tout").cpu().numpy()
    assert not gout[:, 8:11].any() and gout[:, :8].tobytes() == runs[0][0][:, :8].tobytes()
    assert not tout[:11].any() and not tout[13:].any() and tout[11] == rec[2][0] and tout[12] == 3


def test_one_window_carries_the_bits_of_the_plain_accumulator():
    from tests.test_evaluate_gpu import Case as Plain
    B, w, Qw, K, G = 1, 5000, 29, 4096, 40
    b = random_batch(np.random.RandomState(1), B, w, 256, Qw, K)
    c, p = Case(B, w, Qw, K, G), Plain(B, w, 256, Qw, K, 256, False)
    c.put(b, [17])
    p.put(b)
    assert c.launch(c.op()) == 0 and p.launch(p.op()) == 0
    gacc, acc = c.view("gacc").cpu().numpy().reshape(G, 8), p.view("acc").cpu().numpy()
    assert gacc[17, 2:5].tobytes() == acc[2:5].tobytes() and gacc[17, 6].tobytes() == acc[6].tobytes()
    assert np.array_equal(c.view("ghist").cpu().numpy().reshape(G, K)[17], p.view("hist").cpu().numpy())


def test_codes_only_fills_the_large_table():
    B, Qw, K, G = 5, 7, 4096, 251
    c = Case(B, 0, Qw, K, G, codes_only=True)
    rs = np.random.RandomState(9)
    rec = EG.new_record(G, K, B)
    for i, groups in enumerate(([250, 0, 250, 251, 17], [3, 3, 3, 3, 3])):
        b = dict(ind=rs.randint(0, K, B * Qw).astype(np.int64), dist=rs.rand(B * Qw).astype(np.float32))
        b["ind"][2 * Qw:3 * Qw] = K - 1                  # the table's last word, seven times
        c.put(b, groups)
        assert c.launch(c.op()) == 0
        EG.accumulate(*rec, np.asarray(groups, np.int64), ind=b["ind"], dist=b["dist"])
    got = c.got()
    assert got["gacc"] == c.framed("gacc", rec[0]) and got["ghist"] == c.framed("ghist", rec[1].view(np.int32))
    assert got["gtot"] == c.framed("gtot", rec[2]) and got["win"] == c.framed("win", rec[3])
    assert rec[1][250, K - 1] >= 7 and rec[2].tolist() == [1, 2, 0, 0] and not rec[0][:, 1:5].any()
    check_finalize(c, rec)


def test_argument_errors_come_before_any_launch():
    c = Case(2, 96, 12, 64, 3, 16, 64, True)
    c.put(random_batch(np.random.RandomState(0), 2, 96, 16, 24, 64, pitch=64), [0, 2])
    before = c.got()
    v = lambda k: c.view(k).data_ptr()
    bad = [(dict(B=0), L.E_ARG), (dict(G=0), L.E_ARG), (dict(group=None), L.E_ARG), (dict(gacc=None), L.E_ARG),
           (dict(gtot=None), L.E_ARG), (dict(win=None), L.E_ARG), (dict(w=1), L.E_ARG), (dict(w=0), L.E_ARG), (dict(K=0), L.E_ARG),
           (dict(Qw=0), L.E_ARG), (dict(ghist=None), L.E_ARG), (dict(nll=None, ind=None), L.E_ARG), (dict(ptgt=None), L.E_ARG),
           (dict(wav=None), L.E_ARG), (dict(logits=None), L.E_ARG), (dict(n_quant=0), L.E_ARG),
           (dict(gacc=v("gacc") + 4), L.E_ALIGN), (dict(gtot=v("gtot") + 4), L.E_ALIGN), (dict(win=v("win") + 4), L.E_ALIGN),
           (dict(ind=v("ind") + 4), L.E_ALIGN), (dict(group=v("group") + 4), L.E_ALIGN), (dict(nll=v("nll") + 2), L.E_ALIGN),
           (dict(ptgt=v("nll") + 1), L.E_ALIGN), (dict(wav=v("wav") + 2), L.E_ALIGN), (dict(dist=v("dist") + 3), L.E_ALIGN),
           (dict(ghist=v("ghist") + 1), L.E_ALIGN), (dict(logits=v("logits") + 2), L.E_ALIGN)]
    for over, want in bad:
        assert c.launch(c.op(**over)) == want, over
    for over, want in [(dict(G=0), L.E_ARG), (dict(gacc=None), L.E_ARG), (dict(gtot=None), L.E_ARG), (dict(gout=None), L.E_ARG),
                       (dict(tout=None), L.E_ARG), (dict(K=0), L.E_ARG), (dict(scratch=None), L.E_ARG),
                       (dict(gacc=v("gacc") + 4), L.E_ALIGN), (dict(gout=v("gout") + 2), L.E_ALIGN),
                       (dict(tout=v("tout") + 1), L.E_ALIGN), (dict(scratch=v("scratch") + 4), L.E_ALIGN)]:
        assert c.launch(c.op(finalize=True, **over)) == want, over
    assert c.got() == before                             # canaries and contents: nothing ran
    assert c.launch(c.op(w=1, nll=None)) == 0            # codes-only ignores w


# ----------------------------------------------------------------------------------------------
# module surface
# ----------------------------------------------------------------------------------------------
def _voiced(m, B, seed, voices):
    wav, mel, _, jit = _batch(m, B, seed=seed)
    return wav, mel, torch.tensor(voices, device=DEV), jit


def test_grouping_splits_the_plain_record_and_leaves_result_bit_equal():
    hps, m = _tiny()
    K = hps.bn_vq_n_embed
    batches = [_voiced(m, 2, 1, [3, 3]), _voiced(m, 2, 2, [1, 3]), _voiced(m, 1, 3, [4])]     # two batch sizes: the record moves
    with m.evaluation() as ev:
        for b in batches:
            m.evaluate(*b)
        plain = {k: v.cpu().numpy().tobytes() for k, v in ev.result().items()}
    with m.evaluation(by="voice") as ev:
        want = np.zeros((5, K), np.int64)
        for b in batches:
            m.evaluate(*b)
            eng = m._engine
            ind = eng.ind[:eng.Q].view(eng.B, -1).cpu().numpy()
            for i, v in enumerate(b[2].tolist()):
                want[v] += np.bincount(ind[i], minlength=K)
        res, bg, inf, cnt, win = ev.result(), ev.by_group(), ev.information(), ev.counts(), ev.windows()
        assert all(t.device.type == "cuda" and t.shape == (5,) for t in bg.values()) and all(t.dim() == 0 for t in inf.values())
        assert list(bg) == list(L.EVAL_GOUT_NAMES) and list(inf) == list(L.EVAL_TOUT_NAMES)
    eng = m._engine
    assert {k: v.cpu().numpy().tobytes() for k, v in res.items()} == plain
    assert cnt.shape == (5, K) and cnt.dtype == torch.int64 and np.array_equal(cnt.cpu().numpy(), want)
    assert np.array_equal(cnt.sum(0).cpu().numpy(), eng.eval_hist.cpu().numpy().view(np.uint32))
    assert bg["windows"].tolist() == [0, 1, 0, 3, 1] and float(bg["positions"].sum()) == float(res["positions"]) == 5 * 95
    pos = bg["positions"].double()
    mean = float((bg["nll"].double() * pos).sum() / pos.sum())
    print("positions-weighted nll", mean, float(res["nll"]))
    assert abs(mean - float(res["nll"])) <= 1e-6 * float(res["nll"])
    assert float(inf["n"]) == want.sum() and float(inf["batches"]) == 3 and float(inf["groups_used"]) == 3
    gout, tout = EG.finalize(eng.eval_gacc.cpu().numpy(), eng.eval_ghist.cpu().numpy().view(np.uint32), eng.eval_gtot.cpu().numpy())
    for i, name in enumerate(L.EVAL_TOUT_NAMES):
        assert abs(float(inf[name]) - float(tout[i])) <= TOL * max(1.0, abs(float(tout[i]))), name
    assert 0 <= float(inf["mutual_information"]) <= float(inf["group_entropy"]) + TOL
    w = eng.n_win
    nll = eng.dec.nll[:eng.B * w].view(eng.B, w)[:, :w - 1].double().mean(1)              # the last batch, per window
    assert win["nll"].shape == (1,) and abs(float(win["nll"][0]) - float(nll[0])) <= 1e-6 * float(nll[0])


def _trajectory(grouped):
    from ae_wavenet_amd import optim
    hps, m = _tiny()
    opt = optim.FusedAdam(m, lr=1e-3, ema_decay=0.9, max_grad_norm=1.0)
    batch, other = _batch(m, 2), _batch(m, 2, seed=9)
    for step in range(3):
        if grouped:
            with m.evaluation(by="voice") as ev:
                m.evaluate(*other)
                ev.by_group(), ev.information()
            with m.evaluation(groups=2) as ev:
                m.evaluate(*batch, group=torch.tensor([1, 0], device=DEV))
                ev.by_group()
        opt.zero_grad()
        _, _, loss = m.run(*batch)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    eng = m._engine
    n = eng.ps.numel
    state = dict(params=eng.ps.params[:n], m=eng.adam_m[:n], v=eng.adam_v[:n], avg=eng.adam_avg[:n], emb=eng.emb,
                 ema_numer=eng.ema_numer, ema_denom=eng.ema_denom, ind_hist=eng.ind_hist)
    return {k: v.cpu().numpy().tobytes() for k, v in state.items()}, (eng.step_count, eng.avg_steps)


def test_training_trajectory_is_bit_equal_with_grouped_evaluation_in_between():
    plain, cnt_a = _trajectory(False)
    mixed, cnt_b = _trajectory(True)
    assert cnt_a == cnt_b == (3, 3)
    for k in plain:
        assert plain[k] == mixed[k], k


def test_grouped_evaluation_does_not_synchronise_the_host():
    hps, m = _tiny()
    batch = _batch(m, 2)
    with m.evaluation(by="voice") as ev:                 # builds the engine, the plans and the grouped record
        m.evaluate(*batch)
        ev.by_group()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")              # .item() / .cpu() / a blocking copy would raise
    try:
        with m.evaluation(by="voice") as ev:
            m.evaluate(*batch)
            m.evaluate(*batch)
            bg, inf, cnt, win = ev.by_group(), ev.information(), ev.counts(), ev.windows()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(bg["windows"].sum()) == 4 and float(inf["batches"]) == 2 and int(cnt.sum()) == 2 * m._engine.Q


def test_voice_information_of_encoded_codes_equals_the_evaluators():
    hps, m = _tiny()
    K = hps.bn_vq_n_embed
    wav, mel, voice, jit = _voiced(m, 3, 5, [4, 0, 4])
    with m.evaluation(by="voice") as ev:
        m.evaluate(wav, mel, voice, jit)
        inf = {k: v.cpu().numpy().tobytes() for k, v in ev.information().items()}
        cnt = ev.counts().cpu().numpy()
    codes = m.encode(mel)
    got = CD.voice_information(codes, voice, K, hps.n_speakers)
    assert np.array_equal(got.pop("counts").cpu().numpy(), cnt)
    assert {k: v.cpu().numpy().tobytes() for k, v in got.items()} == inf
    flat = CD.voice_information(codes.reshape(-1), voice.repeat_interleave(codes.shape[1]), K, hps.n_speakers)
    assert np.array_equal(flat["counts"].cpu().numpy(), cnt)
    assert float(flat["mutual_information"]) == float(got["mutual_information"]) and float(flat["n"]) == codes.numel()


@pytest.mark.parametrize("kind", ["vae", "ae", "mi"])
def test_models_without_codes_fill_by_group_and_refuse_information(kind):
    if kind == "mi":
        hps, m = _mi()
        wav, mel, _, jit = _mi_batch(m, hps, 2, 2)
    else:
        hps, m = _tiny(kind, bn_n_out=16 if kind == "vae" else 8)
        wav, mel, _, jit = _batch(m, 2)
    voice = torch.tensor([2, 0], device=DEV)
    with m.evaluation() as ev:
        m.evaluate(wav, mel, voice, jit) if kind != "vae" else m.evaluate(wav, mel, voice, jit, eps=torch.zeros(2, m.geom.embed_len, 16, device=DEV))
        plain = float(ev.result()["nll"])
    with m.evaluation(by="voice") as ev:
        m.evaluate(wav, mel, voice, jit) if kind != "vae" else m.evaluate(wav, mel, voice, jit, eps=torch.zeros(2, m.geom.embed_len, 16, device=DEV))
        bg = ev.by_group()
        with pytest.raises(L.AewError):
            ev.information()
    assert bg["windows"].tolist() == [1, 0, 1, 0, 0] and not bg["code_entropy"].any() and not bg["queries"].any()
    assert abs(float(bg["nll"][0] + bg["nll"][2]) / 2 - plain) <= 2e-6 * plain and float(bg["nll"][1]) == 0
