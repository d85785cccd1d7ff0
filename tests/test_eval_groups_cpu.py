"""Evaluation by group without a GPU: the numpy restatement of aew_eval_groups_t (tests/eval_groups_emulator.py) against
independent formulas and known answers; the identities that tie the grouped record to the plain one
(tests/eval_emulator.py); the grouped plans of a TrainEngine built on 'cpu' (the plain evaluation plans untouched, nothing
a training step reads written); the module surface through the CPU plan interpreter; and the data-parallel sum of the
ranks' grouped records over gloo."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, autoencoder_model as ae, config, model as M
from tests import eval_emulator as EE
from tests import eval_groups_emulator as EG
from tests.plan_emulator import Emu
from tests.test_evaluate_cpu import OUTPUTS, EvalEmu, engines, protected, random_batch
from tests.test_plan_cpu import load, tiny_hps


def info(ghist):
    """tout of a table alone, as doubles by name."""
    G = ghist.shape[0]
    _, tout = EG.finalize64(np.zeros((G, EG.GACC_N)), ghist.astype(np.uint32), np.zeros(4))
    return dict(zip(EG.TOUT_NAMES, tout))


def H(p):
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


# ----------------------------------------------------------------------------------------------
# the emulator against independent formulas and known answers
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,K,fill", [(1, 1, 1.0), (3, 7, 0.5), (5, 70, 0.2), (40, 1500, 0.05), (4, 2049, 0.9)])
def test_emulator_information_against_entropies(G, K, fill):
    rs = np.random.RandomState(G * 100 + K)
    tab = (rs.randint(1, 50, (G, K)) * (rs.rand(G, K) < fill)).astype(np.uint32)
    if G > 2:
        tab[1] = 0                                                   # an empty group
    t = info(tab)
    n = tab.astype(np.float64)
    N = n.sum()
    if N == 0:
        assert not any(t.values())
        return
    hc, hg, hcg_joint = H(n.sum(0) / N), H(n.sum(1) / N), H(n.reshape(-1) / N)
    assert t["n"] == N
    assert abs(t["code_entropy"] - hc) < 1e-9 and abs(t["group_entropy"] - hg) < 1e-9
    assert abs(t["mutual_information"] - (hc + hg - hcg_joint)) < 1e-9
    assert abs(t["cond_entropy"] - (hcg_joint - hg)) < 1e-9
    assert t["cells"] == (tab > 0).sum() and t["groups_used"] == (tab.sum(1) > 0).sum() and t["codes_used"] == (tab.sum(0) > 0).sum()
    gout, _ = EG.finalize64(np.zeros((G, 8)), tab, np.zeros(4))
    for g in range(G):
        ng = n[g].sum()
        e = H(n[g] / ng) if ng else 0.0
        assert abs(gout[g, 8] - e) < 1e-9 and gout[g, 10] == (tab[g] > 0).sum()
        assert abs(gout[g, 9] - (2.0 ** e if ng else 0.0)) < 1e-9 * 2.0 ** e


def test_emulator_known_answers():
    t = info(np.outer([1, 2, 3], [2, 4, 6, 8]))                     # independent rows and columns
    assert t["mutual_information"] == 0.0 and t["mi_over_group_entropy"] == 0.0 and t["n"] == 120
    assert (t["cells"], t["groups_used"], t["codes_used"]) == (12, 3, 4)
    # Miller-Madow by hand: (12 - 3 - 4 + 1) / (2 * 120 * ln 2) = 6 / (240 ln 2), subtracted from I = 0: negative, not clamped
    assert t["mutual_information_mm"] == 0.0 - 6.0 / (2.0 * 120.0 * EE.LN2) < 0
    t = info(np.diag([9, 9, 9, 9]))                                  # four voices, one code of their own each
    assert t["mutual_information"] == t["group_entropy"] == t["code_entropy"] == 2.0 and t["cond_entropy"] == 0.0
    assert (t["cells"], t["groups_used"], t["codes_used"]) == (4, 4, 4)
    assert t["mi_over_group_entropy"] == 1.0 and t["mi_over_code_entropy"] == 1.0
    assert t["mutual_information_mm"] == 2.0 - (4 - 4 - 4 + 1) / (2.0 * 36.0 * EE.LN2)      # (-3: the correction adds here)
    tab = np.array([[3, 0, 1], [0, 0, 0], [2, 2, 0]])                # cells 4, rows 2, cols 3, N 8
    t = info(tab)
    assert (t["cells"], t["groups_used"], t["codes_used"], t["n"]) == (4, 2, 3, 8)
    assert abs(t["mutual_information"] - t["mutual_information_mm"] - (4 - 2 - 3 + 1) / (2 * 8 * np.log(2.0))) < 1e-15
    assert not any(info(np.zeros((3, 4))).values())                  # an empty table: x / 0 = 0 throughout


def grouped_batches(rs, B, w, Qw, K, n=3, n_quant=256):
    return [random_batch(rs, B, w, n_quant, B * Qw, K) for _ in range(n)]


def fold(batches, groups, G, K, B):
    rec = EG.new_record(G, K, B)
    for b, g in zip(batches, groups):
        kw = {k: b[k] for k in ("nll", "ptgt", "wav", "tgt_off", "amax", "ind", "dist")}
        EG.accumulate(*rec, np.asarray(g, np.int64), **kw)
    return rec


@pytest.mark.parametrize("B,w,Qw,K,G", [(1, 2, 1, 1, 1), (3, 1030, 5, 70, 5), (4, 40, 3, 16, 3)])
def test_emulator_identities_on_random_batches(B, w, Qw, K, G):
    rs = np.random.RandomState(B * 7 + w)
    batches = grouped_batches(rs, B, w, Qw, K)
    groups = [rs.randint(0, G, B) for _ in batches]
    if B > 1:
        groups[1][0], groups[1][-1] = G, -1                           # two dropped windows
    gacc, ghist, gtot, win = fold(batches, groups, G, K, B)
    assert gacc[:, 0].sum() + gtot[0] == B * gtot[1] and gtot[1] == len(batches)
    assert gtot[0] == (2 if B > 1 else 0) and not gtot[2:].any() and not gacc[:, 7].any()
    acc, hist = np.zeros(16), np.zeros(K, np.uint32)                 # the plain record of the windows that were kept
    n_win = 0
    for b, g in zip(batches, groups):
        keep = (g >= 0) & (g < G)
        n_win += int(keep.sum())
        if keep.any():
            EE.accumulate(acc, hist, b["nll"][keep], b["ptgt"][keep], b["wav"][keep], b["tgt_off"], amax=b["amax"][keep],
                          ind=b["ind"].reshape(B, Qw)[keep].reshape(-1), dist=b["dist"].reshape(B, Qw)[keep].reshape(-1))
    assert np.array_equal(ghist.sum(0), hist)
    assert gacc[:, 1].sum() == n_win * (w - 1) == acc[1] and gacc[:, 5].sum() == n_win * Qw == acc[5]
    assert gacc[:, 4].sum() == acc[4]
    for i, j in ((2, 2), (3, 3), (6, 6)):
        assert abs(gacc[:, i].sum() - acc[j]) <= 1e-12 * abs(acc[j]) + 1e-300
    last = batches[-1]                                               # win: the LAST batch's windows, dropped ones too
    assert win[:, 0].tobytes() == np.array([EE.ordered_sum(last["nll"][b, :w - 1]) for b in range(B)]).tobytes()


def test_emulator_one_window_carries_the_plain_records_bits():
    rs = np.random.RandomState(3)
    for w, Qw in ((2, 1), (1030, 5), (5000, 29)):
        batches = grouped_batches(rs, 1, w, Qw, 64, n=2)
        gacc, ghist, gtot, _ = fold(batches, [[2], [2]], 4, 64, 1)
        acc, hist = np.zeros(16), np.zeros(64, np.uint32)
        for b in batches:
            EE.accumulate(acc, hist, **b)
        assert gacc[2, 2:5].tobytes() == acc[2:5].tobytes() and gacc[2, 6].tobytes() == acc[6].tobytes()
        assert gacc[2, 0] == 2 and gacc[2, 1] == acc[1] and gacc[2, 5] == acc[5] and np.array_equal(ghist[2], hist)
        assert not gacc[[0, 1, 3]].any() and not ghist[[0, 1, 3]].any()


def test_emulator_codes_only_counts_queries_alone():
    rs = np.random.RandomState(4)
    ind = rs.randint(-1, 9, (5, 7)).astype(np.int64)                 # -1 and 8 lie outside [0, 8)
    group = np.array([0, 2, 2, 3, 1], np.int64)                      # 3 is outside [0, 3)
    gacc, ghist, gtot, win = EG.new_record(3, 8, 5)
    EG.accumulate(gacc, ghist, gtot, win, group, ind=ind)
    assert gacc[:, 0].tolist() == [1, 1, 2] and not gacc[:, 1:5].any() and gacc[:, 5].tolist() == [7, 7, 14] and gtot.tolist() == [1, 1, 0, 0]
    for g in range(3):
        rows = ind[group == g].reshape(-1)
        assert np.array_equal(ghist[g], np.bincount(rows[(rows >= 0) & (rows < 8)], minlength=8))
    assert not win.any()


# ----------------------------------------------------------------------------------------------
# plan logic on a CPU engine
# ----------------------------------------------------------------------------------------------
class GroupEmu(EvalEmu):
    """The plan interpreter with the grouped evaluation op (AEW_OP_EVAL_GROUPS) from tests/eval_groups_emulator.py."""

    def _arr(self, ptr, n, shape, dt=None):
        t, o = self.flat(ptr)
        a = t[o:o + n].numpy()                                       # (shares memory: updated in place)
        return (a.view(dt) if dt is not None else a).reshape(shape)

    def op_38(self, p):
        G, K = p.G, p.K
        gacc = self._arr(p.gacc, G * 8, (G, 8))
        ghist = self._arr(p.ghist, G * K, (G, K), np.uint32) if p.ghist else None
        gtot = self._arr(p.gtot, 4, (4,))
        if p.finalize:
            gout, tout = EG.finalize(gacc, ghist, gtot)
            self.wr(p.gout, torch.arange(G * 12), torch.from_numpy(gout.reshape(-1)))
            self.wr(p.tout, torch.arange(16), torch.from_numpy(tout))
            return
        win = self._arr(p.win, p.B * 4, (p.B, 4))
        group = self.rd(p.group, torch.arange(p.B)).numpy()
        kw = {}
        if p.nll:
            n = torch.arange(p.B * p.w)
            kw["nll"] = self.rd(p.nll, n).numpy().reshape(p.B, p.w)
            kw["ptgt"] = self.rd(p.ptgt, n).numpy().reshape(p.B, p.w)
            kw["wav"] = self.rd(p.wav, torch.arange(p.B)[:, None] * p.wav_pitch + torch.arange(p.wav_pitch)[None, :]).numpy()
            kw["tgt_off"] = p.tgt_off
            if p.amax:
                kw["amax"] = self.rd(p.amax, n).numpy().reshape(p.B, p.w)
            else:
                idx = (torch.arange(p.B)[:, None, None] * p.bs + torch.arange(p.w)[None, :, None] * p.pitch
                       + torch.arange(p.n_quant)[None, None, :])
                kw["logits"], kw["n_quant"] = self.rd(p.logits, idx).numpy(), p.n_quant
        if p.ind:
            kw["ind"] = self.rd(p.ind, torch.arange(p.B * p.Qw)).numpy().reshape(p.B, p.Qw)
            kw["dist"] = self.rd(p.dist, torch.arange(p.B * p.Qw)).numpy().reshape(p.B, p.Qw) if p.dist else None
        EG.accumulate(gacc, ghist, gtot, win, group, **kw)


GROUP_OUTPUTS = dict(OUTPUTS)
GROUP_OUTPUTS[L.OP_EVAL_GROUPS] = lambda e, p: [p.gacc, p.ghist, p.gtot, p.win, p.gout, p.tout, p.scratch]
NEW_BUFFERS = {"eval.gacc", "eval.ghist", "eval.gscratch", "eval.gtot", "eval.win", "eval.gout", "eval.tout", "in.group"}


def plan_bytes(pl):
    return bytes(C.string_at(C.addressof(pl.array()), C.sizeof(L.Op) * len(pl.ops))), list(pl.labels)


def test_grouped_plans_leave_the_plain_ones_alone_and_write_no_protected_buffer(golden_dir):
    plain = {name: eng for name, _, eng, _, _ in engines(golden_dir)}            # engines that never group
    for name, z, eng, eps, _ in engines(golden_dir):
        before = [plan_bytes(pl) for pl in (eng.eval_a, eng.eval_b, eng.eval_fin)]
        names = list(eng.ws.bufs)
        assert eng.eval_gfin is None and not any(n.startswith("eval.g") or n in NEW_BUFFERS for n in names), name
        eg, egfin = eng.eval_group_plans(5)
        assert eng.eval_group_plans(5) == (eg, egfin) and eng.eval_G == 5                      # built once
        assert [plan_bytes(pl) for pl in (eng.eval_a, eng.eval_b, eng.eval_fin)] == before, name
        other = plain[name]
        for a, b in ((eng.eval_a, other.eval_a), (eng.eval_b, other.eval_b), (eng.eval_fin, other.eval_fin)):
            assert a.labels == b.labels and [o.kind for o in a.ops] == [o.kind for o in b.ops], name
        assert not any(n.startswith("eval.g") or n in NEW_BUFFERS for n in other.ws.bufs), name
        assert list(other.ws.bufs) == names, name                                  # the parent's allocation list
        assert set(eng.ws.bufs) - set(names) == (NEW_BUFFERS if name == "vqvae-ema" else NEW_BUFFERS - {"eval.ghist", "eval.gscratch"})
        assert eg.labels == ["eval.group_accumulate"] and egfin.labels == ["eval.group_finalize"]
        emu = Emu(eng.ws)
        ranges = {k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in protected(eng).items()}
        ranges.update({k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())        # ... nor the plain record
                       for k, t in (("eval.acc", eng.eval_acc), ("eval.hist", eng.eval_hist), ("eval.out", eng.eval_out))})
        for pl in (eg, egfin):
            for op, lab in zip(pl.array(), pl.labels):
                for ptr in GROUP_OUTPUTS[op.kind](emu, getattr(op.u, L.OP_FIELD[op.kind])):
                    for k, (lo, hi) in ranges.items():
                        assert not (ptr and lo <= ptr < hi), (name, lab, k)
        ev, acc_op = eg.ops[0].u.evg, eng.eval_b.ops[-1].u.eva
        for f in ("nll", "ptgt", "wav", "wav_pitch", "tgt_off", "B", "w", "amax", "logits", "bs", "pitch", "n_quant", "ind", "dist", "K"):
            assert getattr(ev, f) == getattr(acc_op, f), (name, f)                   # the softmax_nll op's pointers
        assert ev.G == 5 and ev.finalize == 0 and egfin.ops[0].u.evg.finalize == 1 and ev.group == eng.in_group.data_ptr()
        assert bool(ev.ind) == bool(ev.ghist) == (name == "vqvae-ema") and (not ev.ind or ev.Qw * ev.B == acc_op.Q)
        eng.eval_group_plans(3)                                                      # another G: built anew
        assert eng.eval_G == 3 and eng.eval_gacc.shape == (3, 8) and eng.eval_g.ops[0].u.evg.G == 3
        assert [plan_bytes(pl) for pl in (eng.eval_a, eng.eval_b, eng.eval_fin)] == before, name


# ----------------------------------------------------------------------------------------------
# the module surface through the interpreter
# ----------------------------------------------------------------------------------------------
def cpu_model(golden_dir, fixture, B=2):
    """(model, engine, inputs) of a golden config with the interpreter in the device's place."""
    z = load(golden_dir, fixture)
    hps, n_mel = tiny_hps(z, global_model="autoencoder")
    torch.manual_seed(11)
    model = ae.AutoEncoder(hps, n_mel=n_mel)
    eng = M.TrainEngine(hps, B=B, device="cpu", n_mel=n_mel, take_compat=True, update_codebook_every_step=False)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: GroupEmu(eng.ws).run(plan)
    model._adopt_engine(eng)           # (what _ensure_engine does once it has an engine: it refuses to build one off the GPU)
    if eng.bn_type == "vqvae-ema":
        eng.emb.copy_(torch.from_numpy(z["emb0"]))
        eng.init_ema_from_emb()
    rs = np.random.RandomState(2)
    g = eng.geom
    def batch():
        return (torch.from_numpy(rs.randint(0, 256, (B, g.enc_in_len)).astype(np.float32)),
                torch.from_numpy(rs.randn(B, n_mel, g.mel_len).astype(np.float32)),
                torch.from_numpy(z["jitter"]))
    return model, eng, batch, hps


def test_surface_by_voice_over_three_batches(golden_dir):
    model, eng, batch, hps = cpu_model(golden_dir, "ae_tiny_vqvae-ema_random.npz")
    G, K, B, w = hps.n_speakers, eng.K, eng.B, eng.n_win
    Qw = eng.Q // B
    data = [batch() for _ in range(3)]
    voices = [torch.tensor(v) for v in ([3, 3], [1, 3], [0, 4])]
    with model.evaluation() as ev:                                   # the same batches without grouping
        for (wav, mel, jit), v in zip(data, voices):
            model.evaluate(wav, mel, v, jit)
        plain = {k: t.clone() for k, t in ev.result().items()}
        with pytest.raises(L.AewError):
            ev.by_group()
    assert eng.eval_gfin is None and not eng.eval_grouping            # nothing grouped was built by a plain block
    with model.evaluation(by="voice") as ev:
        with pytest.raises(L.AewError):
            ev.by_group()                                            # nothing evaluated in this block yet
        want = np.zeros((G, K), np.int64)
        for (wav, mel, jit), v in zip(data, voices):
            model.evaluate(wav, mel, v, jit)
            ind = eng.ind[:eng.Q].numpy().reshape(B, Qw)
            for b in range(B):
                want[int(v[b])] += np.bincount(ind[b], minlength=K)
        res, bg, inf, cnt, win = ev.result(), ev.by_group(), ev.information(), ev.counts(), ev.windows()
    assert not eng.eval_grouping and model._eval_ev is None
    assert set(bg) == set(L.EVAL_GOUT_NAMES) and set(inf) == set(L.EVAL_TOUT_NAMES) and set(win) == {"nll", "top1", "tprb", "dist"}
    for k in plain:                                                  # result() is what it is without grouping, bit for bit
        assert res[k].numpy().tobytes() == plain[k].numpy().tobytes(), k
    assert bg["windows"].tolist() == [1, 1, 0, 3, 1] and bg["positions"].tolist() == [x * (w - 1) for x in (1, 1, 0, 3, 1)]
    assert float(bg["positions"].sum()) == float(res["positions"])
    assert cnt.dtype == torch.int64 and np.array_equal(cnt.numpy(), want)
    assert np.array_equal(cnt.sum(0).numpy(), eng.eval_hist.numpy().view(np.uint32))
    mean = float((bg["nll"].double() * bg["positions"].double()).sum() / bg["positions"].double().sum())
    assert abs(mean / float(res["nll"]) - 1) < 1e-6
    assert float(inf["n"]) == 3 * eng.Q and float(inf["batches"]) == 3 and float(inf["dropped_windows"]) == 0
    assert float(inf["groups_used"]) == 4 and float(inf["cells"]) == (want > 0).sum()
    n = want.astype(np.float64)
    mi = H(n.sum(0) / n.sum()) + H(n.sum(1) / n.sum()) - H(n.reshape(-1) / n.sum())
    assert abs(float(inf["mutual_information"]) - mi) < 1e-6
    acc_nll = eng.dec.nll[:B * w].double().view(B, w)[:, :w - 1].sum(1) / (w - 1)     # the last batch's windows
    assert np.allclose(win["nll"].numpy(), acc_nll.numpy(), rtol=1e-6)
    with model.evaluation(by="voice") as ev:                         # a new block starts at zero
        model.evaluate(*data[0][:2], voices[0], data[0][2])
        assert ev.by_group()["windows"].tolist() == [0, 0, 0, 2, 0] and float(ev.information()["batches"]) == 1


def test_surface_groups_keyword_and_its_errors(golden_dir):
    model, eng, batch, hps = cpu_model(golden_dir, "ae_tiny_vqvae-ema_random.npz")
    wav, mel, jit = batch()
    v = torch.tensor([1, 4])
    epoch = eng.act_epoch
    with pytest.raises(L.AewError):
        model.evaluate(wav, mel, v, jit, group=torch.tensor([0, 1]))                 # group= outside a groups= block
    with model.evaluation() as ev:
        with pytest.raises(L.AewError):
            model.evaluate(wav, mel, v, jit, group=torch.tensor([0, 1]))
    with model.evaluation(by="voice") as ev:
        with pytest.raises(L.AewError):
            model.evaluate(wav, mel, v, jit, group=torch.tensor([0, 1]))
    with model.evaluation(groups=2) as ev:
        with pytest.raises(L.AewError):
            model.evaluate(wav, mel, v, jit)                                         # a missing group=
        with pytest.raises(L.AewError):
            model.evaluate(wav, mel, v, jit, group=torch.tensor([0, 1, 1]))
        assert eng.act_epoch == epoch                                                # ... all before anything ran
        model.evaluate(wav, mel, v, jit, group=torch.tensor([1, 1]))
        model.evaluate(wav, mel, v, jit, group=torch.tensor([0, 2]))                 # 2 lies outside [0, 2): dropped
        bg, inf = ev.by_group(), ev.information()
        assert bg["windows"].tolist() == [1, 2] and float(inf["dropped_windows"]) == 1 and float(inf["batches"]) == 2
        assert ev.counts().shape == (2, eng.K) and int(ev.counts().sum()) == 3 * (eng.Q // eng.B)
    for bad in (dict(by="voice", groups=2), dict(by="gender"), dict(groups=0)):
        with pytest.raises(L.AewError):
            with model.evaluation(**bad):
                pass


def test_surface_without_codes_fills_by_group_and_refuses_information(golden_dir):
    model, eng, batch, hps = cpu_model(golden_dir, "ae_tiny_vae_random.npz")
    wav, mel, jit = batch()
    with model.evaluation(by="voice") as ev:
        model.evaluate(wav, mel, torch.tensor([2, 0]), jit)
        bg = ev.by_group()
        assert bg["windows"].tolist() == [1, 0, 1, 0, 0] and float(bg["nll"][2]) > 0 and not bg["code_entropy"].any()
        assert not bg["queries"].any() and not ev.windows()["dist"].any()
        with pytest.raises(L.AewError):
            ev.information()
        with pytest.raises(L.AewError):
            ev.counts()
        assert eng.eval_ghist is None and not eng.eval_tout[:11].any() and float(eng.eval_tout[12]) == 1


# ----------------------------------------------------------------------------------------------
# data parallel: the ranks' grouped records summed in one all-reduce (two gloo ranks)
# ----------------------------------------------------------------------------------------------
K_DP, G_DP = 64, 3


def _dp_data():
    rs = np.random.RandomState(6)
    return grouped_batches(rs, 2, 33, 6, K_DP, n=4), [rs.randint(0, G_DP + 1, 2) for _ in range(4)]       # (G_DP: dropped)


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    from ae_wavenet_amd import dp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d = dp.DataParallel()
        batches, groups = _dp_data()
        gacc, ghist, gtot, _ = fold(batches[rank * 2:rank * 2 + 2], groups[rank * 2:rank * 2 + 2], G_DP, K_DP, 2)
        big = ghist.copy()
        big[1, 3] += np.uint32(0x90000000)                           # a count past 2^31: the int32 tensor holds unsigned words
        a_t, t_t, h_t = torch.from_numpy(gacc.copy()), torch.from_numpy(gtot.copy()), torch.from_numpy(big.view(np.int32).copy())
        s_acc, s_tot, s_hist = d.sum_eval_group_record(a_t, t_t, h_t)
        assert s_hist.dtype == torch.int64 and s_hist.shape == (G_DP, K_DP) and s_acc.shape == (G_DP, 8)
        assert a_t.numpy().tobytes() == gacc.tobytes() and t_t.numpy().tobytes() == gtot.tobytes() \
            and h_t.numpy().tobytes() == big.tobytes()                                   # arguments left alone
        hps = config.make_hps("vqvae-ema", n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=G_DP,
                              n_blocks=1, n_block_layers=2, enc_n_out=8, bn_n_out=4, bn_vq_n_embed=K_DP, n_win_batch=5)
        eng = M.TrainEngine(hps, B=1, device="cpu", n_mel=5)
        eng._run = lambda plan, timing=False: GroupEmu(eng.ws).run(plan)
        eng.eval_group_reset(G_DP)
        eng.eval_gacc.copy_(a_t)
        eng.eval_gtot.copy_(t_t)
        eng.eval_ghist.copy_(torch.from_numpy(ghist.view(np.int32).copy()))
        gout, tout = d.eval_group_finish(eng)
        assert eng.eval_gacc.numpy().tobytes() == gacc.tobytes() and eng.eval_gtot.numpy().tobytes() == gtot.tobytes() \
            and eng.eval_ghist.numpy().tobytes() == ghist.tobytes()                      # the rank's own record is back
        q.put((rank, s_acc.numpy().copy(), s_tot.numpy().copy(), s_hist.numpy().copy(), gout.numpy().copy(), tout.numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_dp_grouped_record_sum_two_gloo_ranks():
    import torch.multiprocessing as mp
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    batches, groups = _dp_data()
    gacc, ghist, gtot, _ = fold(batches, groups, G_DP, K_DP, 2)      # the single-process record of all batches
    hist = ghist.astype(np.int64)
    for r, s_acc, s_tot, s_hist, gout, tout in res:
        w_gout, w_tout = EG.finalize(s_acc, ghist, s_tot)            # (the summed sums of that rank, the true counts)
        assert gout.tobytes() == w_gout.tobytes() and tout.tobytes() == w_tout.tobytes()
        assert tout[12] == 4 and tout[11] == gtot[0] and tout[0] == hist.sum()
        big = hist.copy()
        big[1, 3] += 2 * 0x90000000
        assert np.array_equal(s_hist, big)
        assert np.array_equal(s_acc[:, [0, 1, 4, 5]], gacc[:, [0, 1, 4, 5]]) and np.array_equal(s_tot, gtot)       # the integer parts
        assert np.all(np.abs(s_acc - gacc) <= 1e-12 * np.abs(gacc))
    for a, b in zip(res[0][1:], res[1][1:]):                         # every rank holds the same sum
        assert a.tobytes() == b.tobytes()


def test_abi_is_appended():
    lib = L.load()
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(32) == C.sizeof(L.EvalGroups) and lib.aew_sizeof(33) == -1
    assert L.OP_EVAL_GROUPS == L.OP_ADAM_GROUPS + 1 and L.OP_FIELD[L.OP_EVAL_GROUPS] == "evg"
    assert lib.aew_sizeof(0) == C.sizeof(L.Op) == 16 + C.sizeof(L.GemmNT)
    assert (L.EVAL_GOUT_NAMES, L.EVAL_TOUT_NAMES) == (EG.GOUT_NAMES, EG.TOUT_NAMES)
