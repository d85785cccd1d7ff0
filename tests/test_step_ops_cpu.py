"""The step's non-GEMM ops one at a time, without a device.

(a) the fp64 definitions of tests/step_ops_reference.py against torch.autograd in float64 (1e-12 relative) and against
    their own adjoint / gradient identities;
(b) the plan interpreter (tests/plan_emulator.py, fp32 torch) on the one-op plans of tests/step_ops_cases.py against
    those definitions, under the derived fp32 rules stated there - the same cases, bytes and rules the kernels are held
    to in tests/test_step_ops_gpu.py (whose rules for __expf / __logf outputs are measured constants instead);
(c) the launcher's contract for aew_softmax_nll_t.peak / amax: refused outside the 256-class register form.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Plan
from tests import step_ops_cases as K
from tests import step_ops_reference as R
from tests.plan_emulator import Emu

RTOL = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-300)
    assert float(np.abs(a - b).max()) <= RTOL * scale, (what, float(np.abs(a - b).max()), scale)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


# =================================================================================================
# (a) the references are right
# =================================================================================================
def test_storage_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, 1e-40, 0.0, 257.0, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()       # torch's conversion is round-to-nearest-even
    assert (R.rne_bf16(x).view(np.uint32) == want.view(np.uint32)).all()
    rng = np.random.default_rng(0)
    y = (rng.standard_normal(4096) * 10.0 ** rng.integers(-20, 20, 4096)).astype(np.float32)
    assert (R.rne_bf16(y).view(np.uint32) == torch.from_numpy(y).to(torch.bfloat16).float().numpy().view(np.uint32)).all()
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert R.rne_bf16(np.float32(1.00390625)) == 1.0 and R.rne_bf16(np.float32(1.01171875)) == np.float32(1.015625)
    assert R.f32(0.1).dtype == np.float32 and float(R.f32(0.1)) == float(np.float32(0.1))


@pytest.mark.parametrize("gmul", [None, 0.37])
def test_ref_softmax_nll_vs_autograd(gmul):
    rng = np.random.default_rng(1)
    B, w, Q, Qp, off = 3, 9, 20, 24, 2
    lg = rng.uniform(-4, 4, (B, w, Q))
    lg[0, 1] = np.linspace(-80, 80, Q)
    wav = rng.integers(0, Q, (B, w + 5))
    x = _t(lg, True)
    lsm = torch.log_softmax(x, -1)
    tgt = torch.from_numpy(wav[:, off + 1: off + w]).long()
    lp = torch.gather(lsm[:, :w - 1], 2, tgt[..., None])[..., 0]
    nll, ptgt, peak, amax = R.softmax_nll_fwd(lg, wav, off)
    _close(nll[:, :w - 1], -lp.detach().numpy(), "nll")
    _close(ptgt[:, :w - 1], lp.exp().detach().numpy(), "ptgt")
    _close(peak, lsm.max(-1)[0].detach().numpy(), "peak")
    assert (amax == lsm.argmax(-1).numpy()).all() and (nll[:, w - 1] == 0).all() and (ptgt[:, w - 1] == 0).all()
    scale = 1.0 / 24
    (-lp.sum() * scale * (gmul or 1.0)).backward()
    ref = R.softmax_nll_bwd(lg, wav, off, scale, Qp, gmul)
    _close(ref[:, :, :Q], x.grad.numpy(), "dlogits")
    assert (ref[:, :, Q:] == 0).all() and (ref[:, w - 1] == 0).all() and not np.signbit(ref[:, w - 1]).any()
    tie = np.zeros((1, 2, 8))
    tie[0, 0, [2, 6]] = 3.0
    assert R.softmax_nll_fwd(tie, np.zeros((1, 4), dtype=np.int64), 0)[3][0, 0] == 2        # the lowest class of a tie


@pytest.mark.parametrize("metric", [0, 1])
def test_ref_vq_bwd_vs_autograd(metric):
    rng = np.random.default_rng(2)
    Q, Kc, d = 7, 5, 6
    z, emb, dzq = rng.standard_normal((Q, d)), rng.standard_normal((Kc, d)), rng.standard_normal((Q, d))
    ind = rng.integers(0, 3, Q)
    coef, dcoef, gm = 0.25, 0.7, 0.37
    zt, et = _t(z, True), _t(emb, True)
    c = et[torch.from_numpy(ind)]
    t = zt - c.detach()
    if metric == 0:
        dist = (t * t).sum(-1).sqrt() / ((zt * zt).sum(-1).sqrt() + (c.detach() ** 2).sum(-1).sqrt())
    else:
        dist = (t * t).sum(-1)
    _close(R.vq_dist(z, emb[ind], metric), dist.detach().numpy(), "dist")
    l2 = ((zt.detach() - c) ** 2).sum()                       # the l2 term of vq_bn.py:78 (stop-gradient on ze)
    (coef * gm * dist.sum() + dcoef * gm * l2 + (zt * _t(dzq)).sum()).backward()
    demb0 = rng.standard_normal((Kc, d))
    dze, demb = R.vq_bwd(z, emb, ind, dzq, metric, coef, dcoef, gm, demb0)
    _close(dze, zt.grad.numpy(), "dze")
    _close(demb - demb0, et.grad.numpy(), "demb")
    assert (demb[3:] == demb0[3:]).all()                      # codes nobody chose: untouched
    # the guarded points: z == code gives no first term, z == 0 no second
    z2 = z.copy()
    z2[0], z2[1] = emb[ind[0]], 0.0
    t1, t2 = R.vq_bwd_terms(z2, emb, ind, 0)
    assert (t1[0] == 0).all() and (t2[0] == 0).all() and (t2[1] == 0).all() and np.isfinite(t1).all() and np.isfinite(t2).all()
    _close(t1[1], -emb[ind[1]] / (emb[ind[1]] ** 2).sum(), "first term at the zero row")


@pytest.mark.parametrize("gate", [None, "below", "above"])
def test_ref_vae_vs_autograd(gate):
    rng = np.random.default_rng(3)
    Q, d = 4, 6
    mu, ls, eps, ds = (rng.standard_normal((Q, d)) for _ in range(4))
    klc, gm, free = 0.013, 0.37, 2.0
    m, s = _t(mu, True), _t(ls, True)
    smp = m + torch.exp(0.5 * s) * _t(eps)
    terms = (1 + s - m * m - torch.exp(s)).sum(-1)
    rs, rk = R.vae_fwd(mu, ls, eps)
    _close(rs, smp.detach().numpy(), "sample")
    _close(rk, terms.detach().numpy(), "kl_terms")
    kl = -0.5 * terms.sum()
    kv = None if gate is None else (free - 1e-3 if gate == "below" else free + 1e-3)
    # the gate is the backward of torch.clamp(kl, min=free_nats) at the value kl_value
    klg = kl if kv is None else torch.clamp(kl - kl.detach() + kv, min=free)
    ((smp * _t(ds)).sum() + klc * gm * klg).backward()
    dmu, dls = R.vae_bwd(mu, ls, eps, ds, klc, gm, kv, free)
    _close(dmu, m.grad.numpy(), "dmu")
    _close(dls, s.grad.numpy(), "dls")


def test_ref_ae_norm_vs_autograd():
    rng = np.random.default_rng(4)
    z = rng.standard_normal((4, 6))
    z[0] *= 0.5 / np.linalg.norm(z[0])
    z[1] *= 1.7 / np.linalg.norm(z[1])
    din = rng.standard_normal((4, 6))
    zt = _t(z, True)
    term = ((zt * zt).sum(-1).sqrt() - 1).abs()
    _close(R.ae_norm_fwd(z), term.detach().numpy(), "term")
    (0.6 * 0.37 * term.sum() + (zt * _t(din)).sum()).backward()
    _close(R.ae_norm_bwd(z, din, 0.6, 0.37), zt.grad.numpy(), "dze")
    e = np.zeros((2, 6))
    e[0, 2] = -1.0                                            # norm exactly 1: sgn = 0; norm 0: no term
    assert (R.ae_norm_bwd(e, din[:2], 0.6) == din[:2]).all() and (R.ae_norm_fwd(e) == [0.0, 1.0]).all()


@pytest.mark.parametrize("spk_b,running,rng_", [(True, 0, None), (False, 2, None), (True, 2, (1, 2))])
def test_ref_spk_bwd_is_the_gradient_of_spk_bias(spk_b, running, rng_):
    case = K.SpkCase(40, 48, 4, 5, spk_b=spk_b, running=running, backward=True)
    case.build()
    gc = R.spk_gc(case.params, case.voice, case.off_spk_w, case.off_spk_b, case.G, case.n_speakers)
    cs = R.spk_colsum_per_element(case.colsum, running)
    if running:                                               # running sums, differenced: the per-element values
        _close(np.cumsum(cs[:, :running], axis=0), case.colsum[:, :running].astype(np.float64), "running sums")
    first, count = rng_ or (0, case.Lr)
    p = _t(case.params, True)
    bias = _spk_bias_torch(case, p)
    mask = torch.zeros(bias.shape, dtype=torch.float64)
    mask[:, first:first + count] = 1
    (bias * mask * _t(cs)).sum().backward()
    g0 = case.g0.astype(np.float64)
    got = R.spk_bwd(case.params, case.voice, *case.args, cs, gc, g0, first, None if rng_ is None else count)
    bp, spk, present = case.regions()
    grad = p.grad.numpy()
    covered = np.zeros(g0.size, dtype=bool)
    for l in range(first, first + count):                     # bias / projection gradients of the op's layers: overwritten
        for gate in (0, 1):
            ob, ov = case.off_bias[gate][l], case.off_proj[gate][l]
            sel = [ov + K.grid((case.D, case.C_lc + case.G), (case.G, 1)).reshape(-1) + case.C_lc] + ([ob + np.arange(case.D)] if ob >= 0 else [])
            for s in sel:
                _close(got[s], grad[s], "bias / projection gradient")
                covered[s] = True
    for s in spk:                                             # speaker rows: added to what was there
        _close(got[s] - g0[s], grad[s], "speaker-embedding gradient")
        covered[s] = True
    assert (got[~covered] == g0[~covered]).all()              # everything else untouched: other layers, absent speaker, C_lc columns
    assert 2 not in present


def _spk_bias_torch(case, p):
    """spk_bias restated in torch float64 on a flat parameter tensor (for autograd)"""
    G, D, Cc = case.G, case.D, case.C_lc + case.G
    gc = p[case.off_spk_w: case.off_spk_w + G * case.n_speakers].view(G, case.n_speakers)[:, torch.from_numpy(case.voice)].t()
    if case.off_spk_b >= 0:
        gc = gc + p[case.off_spk_b: case.off_spk_b + G][None, :]
    rows = []
    for l in range(case.Lr):
        row = torch.zeros(case.B, 2 * case.D_pad, dtype=torch.float64)
        for gate in (0, 1):
            ov, ob = case.off_proj[gate][l], case.off_bias[gate][l]
            v = gc @ p[ov: ov + D * Cc].view(D, Cc)[:, case.C_lc:].t()
            if ob >= 0:
                v = v + p[ob: ob + D][None, :]
            idx = torch.from_numpy(R.pack_index(np.arange(D), gate))
            row = row.index_add(1, idx, v)
        rows.append(row)
    ref, _ = R.spk_bias(case.params, case.voice, *case.args)
    out = torch.stack(rows, 1)
    _close(ref, out.detach().numpy(), "spk_bias")
    return out


@pytest.mark.parametrize("take", [0, 1])
@pytest.mark.parametrize("B,N,C", [(1, 7, 3), (3, 7, 8), (5, 29, 3), (5, 1, 3)])
def test_ref_lc_scatter_is_the_adjoint_of_gather(take, B, N, C):
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((B, N, C)), rng.standard_normal((B, N, C))
    jit = K.jitter_rows(rng, B, N, N + 5, shift=2)
    _close((R.lc_gather_f64(x, jit, take) * y).sum(), (x * R.lc_scatter(y, jit, take)).sum(), "adjoint")
    # the clamp, and torch.take itself on the (B, C, N) tensor
    jc = np.clip(jit[:, :N], 0, N - 1)
    if take:
        ncl = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1)))
        want = torch.take(ncl, torch.from_numpy(np.arange(B)[:, None] * N + jc)).numpy()[:, :, None].repeat(C, 2)
    else:
        want = np.take_along_axis(x, jc[:, :, None].repeat(C, 2), 1)
    assert (R.lc_gather_f64(x, jit, take) == want).all()
    g = R.lc_gather(x.astype(np.float32), jit, C + 5, take)
    assert (g[:, :, C:] == 0).all() and (g[:, :, :C] == R.rne_bf16(want.astype(np.float32))).all()


def test_ref_base_gather_is_one_add():
    rng = np.random.default_rng(6)
    W, b = rng.standard_normal((5, 8)).astype(np.float32), rng.standard_normal(5).astype(np.float32)
    wav = np.array([[9, 9, 9, 0, 7, 3]])
    x, oh = R.base_gather(wav, 3, 3, W, b, 8, True, 16)
    want = (torch.from_numpy(W.T[[0, 7, 3]]) + torch.from_numpy(b)).to(torch.bfloat16).float().numpy()
    assert (x[0, :, :5] == want).all() and (x[0, :, 5] == 1).all() and (x[0, :, 6:] == 0).all()
    assert (oh.argmax(-1) == [[0, 7, 3]]).all() and (oh.sum(-1) == 1).all()
    assert (R.base_gather(wav, 3, 3, W, None, 8, False)[0][0, :, 5:] == 0).all()


# =================================================================================================
# (b) the interpreter against the references
# =================================================================================================
def run_emu(case):
    ws = case.build()
    before = K.snapshot(ws)
    plan = Plan(case.name)
    for kind, payload, label in case.ops(ws):
        plan.add(kind, payload, label)
    Emu(ws).run(plan)
    K.verify(case, before, K.snapshot(ws), what="interpreter")


@pytest.mark.parametrize("case", K.softmax_cases(), ids=lambda c: c.name)
def test_emu_softmax_nll(case):
    run_emu(case)


@pytest.mark.parametrize("T", K.BASE_T)
@pytest.mark.parametrize("R_,R_pad", K.BASE_R)
def test_emu_base_gather(T, R_, R_pad):
    for with_wt, without in K.base_gather_variants(T, R_, R_pad):
        run_emu(with_wt)


@pytest.mark.parametrize("B,N,C,Cp", K.LC_SHAPES)
def test_emu_lc_gather_scatter(B, N, C, Cp):
    for case in K.lc_cases(B, N, C, Cp):
        run_emu(case)


@pytest.mark.parametrize("case", K.lc_big_cases(), ids=lambda c: c.name)
def test_emu_lc_scatter_both_forms(case):
    run_emu(case)


@pytest.mark.parametrize("D,Dp,G,B", K.SPK_SHAPES)
def test_emu_spk_bias_and_bwd(D, Dp, G, B):
    for i, (spk_b, running) in enumerate(K.SPK_VARIANTS):
        run_emu(K.SpkCase(D, Dp, G, B, spk_b=spk_b))
        run_emu(K.SpkCase(D, Dp, G, B, spk_b=spk_b, running=running, backward=True, split=bool(i & 1)))


@pytest.mark.parametrize("Q,d,dp,metric", K.VQ_SHAPES)
def test_emu_vq_bwd(Q, d, dp, metric):
    for demb, gmul in K.VQ_VARIANTS:
        run_emu(K.VqBwdCase(Q, d, dp, metric, demb, gmul))


@pytest.mark.parametrize("Q,d,dp", K.ROW_SHAPES)
def test_emu_vae_and_ae_norm(Q, d, dp):
    for case in K.vae_cases(Q, d, dp) + K.ae_norm_cases(Q, d, dp):
        run_emu(case)


def test_reference_needs_no_exclusion():
    """Every expectation of every case is finite and covers each written element once: no case or element is masked."""
    cases = K.softmax_cases() + [c for v in K.base_gather_variants(5, 24, 32) for c in v] + K.lc_cases(3, 7, 3, 8) + K.lc_big_cases()
    cases += [K.SpkCase(40, 48, 4, 33, backward=bw, running=2) for bw in (False, True)]
    cases += [K.VqBwdCase(Q, 100, 128, m, True, 0.37) for Q in (1, 5, 130) for m in (0, 1)] + K.vae_cases(5, 100, 128) + K.ae_norm_cases(5, 16, 16)
    cases += K.ae_norm_cases(1, 64, 64) + K.ae_norm_cases(1, 100, 128) + [K.VqBwdCase(1, 16, 16, 0, True)]
    for case in cases:
        case.build()
        for e in case.expect():
            assert np.isfinite(e.ref.astype(np.float64)).all(), (case.name, e.tag)
            assert e.S is None or not np.isnan(e.S).any(), (case.name, e.tag)


# =================================================================================================
# (c) the launcher's contract for peak / amax
# =================================================================================================
def _peak_supported(Q, Q_pad, pitch, bs):
    """the predicate of k_softmax_nll's register path, the only one that writes peak / amax"""
    return Q == 256 and Q_pad == 256 and pitch % 4 == 0 and bs % 4 == 0


def _softmax_record(host, Q, Q_pad, pitch, bs, peak=True, amax=True, backward=0):
    op = L.Op()
    op.kind = L.OP_SOFTMAX_NLL
    sm = op.u.sm
    base = (C.addressof(host) + 63) & ~63
    sm.logits, sm.wav, sm.nll, sm.ptgt, sm.dlogits = base, base + 1024, base + 2048, base + 3072, base + 4096
    sm.peak, sm.amax = (base + 5120) if peak else None, (base + 6144) if amax else None
    sm.bs, sm.pitch, sm.wav_pitch, sm.tgt_off = bs, pitch, 16, 0
    sm.B, sm.w, sm.Q, sm.Q_pad, sm.backward = 1, 2, Q, Q_pad, backward
    sm.dl_bs, sm.dl_pitch = 2 * Q_pad, Q_pad
    return op


def test_softmax_peak_outside_the_register_form_is_refused_before_any_launch():
    lib = L.load()
    host = (C.c_uint8 * (8192 + 64))()
    shapes = [(64, 64, 64, 128), (100, 128, 128, 256), (16, 64, 64, 128), (320, 320, 320, 640), (256, 256, 258, 516),
              (256, 256, 257, 516), (256, 256, 256, 514), (256, 384, 384, 768), (255, 256, 256, 512), (128, 256, 256, 512)]
    for Q, Qp, pitch, bs in shapes:
        assert not _peak_supported(Q, Qp, pitch, bs)
        for kw in (dict(), dict(peak=False), dict(amax=False)):
            fail = C.c_int(-1)
            op = _softmax_record(host, Q, Qp, pitch, bs, **kw)
            want = L.E_UNSUP if not kw else L.E_ARG          # one of the two alone is malformed wherever it is asked for
            assert lib.aew_run_plan(C.byref(op), 1, None, C.byref(fail)) == want, (Q, Qp, pitch, bs, kw)
            assert fail.value == 0
    fail = C.c_int(-1)                                        # the supported shape with only one of the two arrays
    assert lib.aew_run_plan(C.byref(_softmax_record(host, 256, 256, 256, 512, amax=False)), 1, None, C.byref(fail)) == L.E_ARG
    assert bytes(host) == bytes(8192 + 64)                    # nothing written
    with pytest.raises(RuntimeError):                         # the interpreter keeps the same contract
        run_emu(K.SoftmaxCase(64, 64, 64, False, peak=True))
    with pytest.raises(RuntimeError):
        run_emu(K.SoftmaxCase(256, 256, 258, False, peak=True))


@pytest.mark.parametrize("n_quant", [256, 64, 100, 320])
def test_model_asks_for_peak_exactly_where_the_launcher_accepts_it(n_quant):
    from ae_wavenet_amd import config, model as M
    hps = config.make_hps("vqvae-ema", n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=3, n_blocks=1,
                          n_block_layers=2, enc_n_out=8, bn_n_out=4, bn_vq_n_embed=16, n_win_batch=6, n_quant=n_quant)
    eng = M.TrainEngine(hps, B=2, device="cpu", n_mel=5)
    sm = eng.dec._softmax(False, 0.0)
    assert bool(sm.peak) == bool(sm.amax) == _peak_supported(sm.Q, sm.Q_pad, sm.pitch, sm.bs), (sm.Q, sm.Q_pad, sm.pitch, sm.bs)
    if not sm.peak:                                           # and the launcher refuses what the model does not ask for
        host = (C.c_uint8 * (8192 + 64))()
        fail = C.c_int(-1)
        op = _softmax_record(host, sm.Q, sm.Q_pad, sm.pitch, sm.bs)
        assert L.load().aew_run_plan(C.byref(op), 1, None, C.byref(fail)) == L.E_UNSUP
