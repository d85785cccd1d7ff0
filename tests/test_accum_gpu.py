"""Gradient accumulation on the GPU: the AEW_OP_ACCUM kernels through ctypes -> C ABI against numpy fp32, and the module
surface with `accumulate=k` at full width: the group's gradient is the fp32 sequential sum of the micro-batches' own
gradients bit for bit, the EMA runs once on the summed statistics, the step is a plain engine's step on that sum with
grad_scale / k, and the whole group stands against the fp32 torch oracle on the batch made of its micro-batches."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd import model as M
from tests.accum_emulator import ADD, FIRST, LAST, fold, sequential_sum
from tests.test_gpu_parity import REL_L2_MEDIAN, REL_L2_WORST, seeded_full_engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = -12345.5
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 7 * 1024 + 2]
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()


def same(got, want):
    """Bit equality, NaN compared by position."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        got[~nan].tobytes() == want[~nan].tobytes()


# ----------------------------------------------------------------------------------------------
# A. the op
# ----------------------------------------------------------------------------------------------
def _rc(acc, g, n, mode):
    op = L.Op()
    op.kind = L.OP_ACCUM
    a = op.u.accum
    a.acc, a.g, a.n, a.mode = acc, g, n, mode
    fail = C.c_int(-1)
    rc = L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
    torch.cuda.synchronize()
    return rc


def _values(n, i):
    """Magnitudes 1e-30 .. 1e30 with random signs; +-0, +-inf and nan at the head and in the scalar tail, rotated by i so
    that the chain meets every pair of them."""
    rs = np.random.RandomState(100 * n + i)
    x = (rs.choice([-1.0, 1.0], n) * 10.0 ** rs.uniform(-30, 30, n)).astype(np.float32)
    for j in range(min(n, 10)):
        x[j] = SPECIAL[(j * (i + 1) + i) % 5]
    for j in range(min(max(n - 10, 0), 5)):
        x[n - 1 - j] = SPECIAL[(j + 2 * i) % 5]
    if n >= 1023:                                                   # every ordered pair of them meets in FIRST -> ADD
        x[100:125] = SPECIAL[np.arange(25) % 5] if i % 2 == 0 else SPECIAL[np.arange(25) // 5]
    return x


@pytest.mark.parametrize("n", SIZES)
def test_op_chain_against_numpy(n):
    assert L.load().aew_sizeof(25) == C.sizeof(L.Accum) and L.load().aew_abi_version() == 28
    bufs = [torch.full((n + 12,), CANARY, device=DEV) for _ in range(2)]
    acc, g = bufs[0][4:4 + n], bufs[1][4:4 + n]                      # 16 bytes into the allocations: aligned
    want_acc = np.full(n, CANARY, np.float32)
    for i, mode in enumerate((FIRST, ADD, ADD, LAST)):
        x = _values(n, i)
        g.copy_(torch.from_numpy(x))
        assert _rc(acc.data_ptr() if n else None, g.data_ptr() if n else None, n, mode) == 0
        want_acc, want_g = fold(want_acc, x, mode)
        assert same(acc.cpu().numpy(), want_acc), (n, i)
        assert same(g.cpu().numpy(), want_g), (n, i)
        if mode == LAST:
            assert same(want_g, sequential_sum([_values(n, k) for k in range(4)]))
        else:
            assert bits(g) == x.tobytes()                              # FIRST / ADD leave g alone, bit for bit
        for b in bufs:
            c = b.cpu().numpy()
            assert (c[:4] == CANARY).all() and (c[4 + n:] == CANARY).all()
    if n >= 5:
        assert np.isnan(want_acc).any()
    if n >= 1023:
        z = want_acc[100:125]
        assert np.isinf(z).any() and (z == 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()


def test_op_refusals_write_nothing():
    n = 1025
    bufs = [torch.full((2 * n + 16,), CANARY, device=DEV) for _ in range(2)]
    a, g = bufs[0].data_ptr(), bufs[1].data_ptr()
    cases = [((a, g, -1, ADD), L.E_ARG), ((None, g, n, ADD), L.E_ARG), ((a, None, n, FIRST), L.E_ARG),
             ((a, g, n, -1), L.E_ARG), ((a, g, n, 3), L.E_ARG), ((a, a, n, ADD), L.E_ARG),
             ((a, a + 4096, n, LAST), L.E_ARG), ((a + 4096, a, n, FIRST), L.E_ARG),
             ((a + 4, g, n, ADD), L.E_ALIGN), ((a, g + 8, n, LAST), L.E_ALIGN), ((a + 2, g, n, FIRST), L.E_ALIGN)]
    for args, want in cases:
        assert _rc(*args) == want, args
    assert _rc(None, None, 0, ADD) == 0 and _rc(a, g, 0, LAST) == 0     # n = 0: a no-op
    for b in bufs:
        assert (b.cpu().numpy() == CANARY).all()
    # buffers that touch without overlapping are accepted
    t = torch.zeros(2 * 1024, device=DEV)
    t[1024:] = 1.0
    assert _rc(t.data_ptr(), t.data_ptr() + 4 * 1024, 1024, ADD) == 0
    assert float(t[:1024].sum()) == 1024.0 and float(t[1024:].sum()) == 1024.0


# ----------------------------------------------------------------------------------------------
# B / D. full width: vqvae-ema, B = 1, w = 100, k = 2 - the two rows of the B = 2 batch of tests/test_gpu_parity.py
# ----------------------------------------------------------------------------------------------
LR = 1e-4


def _reseed(eng, wts, emb):
    n = eng.ps.numel
    for k, v in wts.items():
        eng.ps.view(k).copy_(torch.from_numpy(v))
    eng.emb.copy_(torch.from_numpy(emb))
    eng.init_ema_from_emb()
    zero = torch.zeros(n)
    eng.load_opt_state(M.OptState(0, zero, zero))


@pytest.fixture(scope="module")
def full():
    """Built once and left unchanged: the B = 2 engine and inputs, and - from a plain B = 1 engine with the same weights
    and codebook - every row's own gradient, statistics and code indices."""
    hps, e2, wts, emb, inp = seeded_full_engine(B=2, w=100)
    _, e1, _, _, _ = seeded_full_engine(B=1, w=100)
    rows = [[t[j:j + 1].to(DEV) for t in inp] for j in range(2)]
    n, own = e1.ps.numel, []
    for r in rows:
        e1.init_ema_from_emb()
        e1.set_inputs(*r)
        e1.forward()
        e1.backward()
        torch.cuda.synchronize()
        own.append((e1.ps.grads[:n].cpu().numpy().copy(), e1.zn_sum.cpu().numpy().copy(), e1.ind[:e1.Q].cpu().numpy().copy()))
    return dict(hps=hps, e2=e2, e1=e1, wts=wts, emb=emb, inp=inp, rows=rows, own=own)


def _accum_model(full, k=2):
    from ae_wavenet_amd import autoencoder_model as ae
    torch.manual_seed(1)
    m = ae.AutoEncoder(full["hps"], n_mel=39, update_codebook_every_step=False, accumulate=k).to(DEV)
    _, eng, _, _, _ = seeded_full_engine(B=1, w=100)
    m._adopt_engine(eng)
    _reseed(eng, full["wts"], full["emb"])
    return m, eng


@pytest.mark.parametrize("opts", [{}, dict(max_grad_norm=1.0, track_update_ratio=True, ema_decay=0.9)], ids=["plain", "clip+track+avg"])
def test_full_width_group_is_the_sequential_sum(full, opts):
    from ae_wavenet_amd import optim
    m, eng = _accum_model(full)
    opt = optim.FusedAdam(m, lr=LR, **opts)
    n, own = eng.ps.numel, full["own"]
    p0 = bits(eng.ps.params[:n])
    opt.zero_grad()
    m.run(*full["rows"][0])[2].backward()
    assert bits(eng.ps.grads[:n]) == own[0][0].tobytes() and bits(eng.zn_sum) == own[0][1].tobytes()
    assert (m.micro_step, m.group_ready) == (1, False)
    opt.step()                                                          # inside the group: a no-op
    assert bits(eng.ps.params[:n]) == p0 and eng.step_count == 0 and not eng.adam_m[:n].any()
    opt.zero_grad()
    m.run(*full["rows"][1])[2].backward()
    torch.cuda.synchronize()
    g_sum = sequential_sum([own[0][0], own[1][0]])
    zn = sequential_sum([own[0][1], own[1][1]])
    assert (m.micro_step, m.group_ready) == (0, True)
    assert bits(eng.ps.grads[:n]) == g_sum.tobytes()
    assert bits(eng.acc_grads[:n]) == own[0][0].tobytes()
    assert bits(eng.zn_sum) == zn.tobytes() and zn[eng.z_sum.numel():].sum() == 2 * eng.Q
    # ONE EMA on the summed statistics: the plain engine's own EMA plan from the same start
    e1 = full["e1"]
    _reseed(e1, full["wts"], full["emb"])
    e1.zn_sum.copy_(torch.from_numpy(zn))
    e1.ema_plan.run(stream())
    assert bits(eng.ema_numer) == bits(e1.ema_numer) and bits(eng.ema_denom) == bits(e1.ema_denom)
    # the step: the plain engine's, its gradient buffer loaded with the sum, grad_scale = 0.5
    opt.step()
    e1.ps.grads[:n].copy_(torch.from_numpy(g_sum))
    kw = dict(max_grad_norm=1.0, track=True, avg_rate=optim.ema_rate_at(0.9, 0)) if opts else {}
    e1.adam_step(LR, 0.5, **kw)
    torch.cuda.synchronize()
    assert (eng.step_count, m.group_ready) == (1, False) and bits(eng.ps.params[:n]) != p0
    for name in ("adam_m", "adam_v") + (("adam_avg",) if opts else ()):
        assert bits(getattr(eng, name)[:n]) == bits(getattr(e1, name)[:n]), name
    assert bits(eng.ps.params[:n]) == bits(e1.ps.params[:n])
    if opts:
        assert bits(eng.clip_out[:4]) == bits(e1.clip_out[:4]) and bits(eng.update_ratios()) == bits(e1.update_ratios())
        print(f"group norm {float(eng.clip_out[0]):.4f}, clip coefficient {float(eng.clip_out[1]):.4f}")
    else:
        assert eng.adam_avg is None


def _against(grads, ref):
    """The comparison of tests/test_gpu_parity.py::test_full_width_step_vs_oracle: per tensor the max-normalised error and
    the cosine (asserted there and here), and the list of relative L2 errors."""
    rl2 = []
    for k, got in grads.items():
        r = ref[k]
        if r is None or r.abs().max().item() == 0:
            continue
        e = (got - r).abs().max().item() / r.abs().max().item()
        cos = torch.nn.functional.cosine_similarity(got.flatten(), r.flatten(), dim=0).item()
        assert e < 0.15 and cos > 0.99, (k, e, cos)
        rl2.append(((got - r).norm().item() / r.norm().item(), k))
    rl2.sort()
    return rl2[len(rl2) // 2][0], rl2[-1][0], rl2[-1][1]


def test_group_against_the_oracle_on_the_whole_batch(full):
    """Two micro-batches of B = 1 are the rows of one B = 2 batch; the fp32 torch oracle runs that batch.  The vqvae-ema
    loss is a SUM over windows (rec.sum() + com.sum()), so the oracle's gradient is the group's sum and `.grad / 2` - the
    mean FusedAdam steps on - stands against the oracle's gradient / 2; the bounds are relative, those of
    tests/test_gpu_parity.py::test_full_width_step_vs_oracle as asserted there.  Measured on an MI355X (deterministic
    kernels): relative L2 median / worst one batch 0.0841 / 0.1047, accumulated 0.0841 / 0.1047
    (worst: decoder.base_layer.weight on both paths)."""
    from oracle import ref_model as R
    hps, e2, wts, emb, inp = (full[k] for k in ("hps", "e2", "wts", "emb", "inp"))
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in wts.items()}
    out = R.ae_run(sd, {"emb": torch.from_numpy(emb)}, hps, e2.geom, *inp, loss_mode="intended", take_compat=False)
    out["loss"].backward()
    ref_ind = out["min_ind"].numpy()
    # the parent path: the batch in one piece
    _reseed(e2, wts, emb)
    e2.set_inputs(*[t.to(DEV) for t in inp])
    e2.forward()
    e2.backward()
    torch.cuda.synchronize()
    assert np.array_equal(e2.ind[:e2.Q].cpu().numpy(), ref_ind.reshape(-1))
    one = _against({k: e2.ps.view(k, grad=True).cpu() for k in e2.ps.names()}, {k: sd[k].grad for k in sd})
    # the accumulated path
    m, eng = _accum_model(full)
    for j, row in enumerate(full["rows"]):
        m.zero_grad()
        m.run(*row)[2].backward()
        torch.cuda.synchronize()
        assert np.array_equal(eng.ind[:eng.Q].cpu().numpy(), ref_ind[j].reshape(-1)), f"code indices of micro-batch {j}"
    acc = _against({k: eng.ps.view(k, grad=True).cpu() / 2 for k in eng.ps.names()},
                   {k: None if sd[k].grad is None else sd[k].grad / 2 for k in sd})
    print(f"relative L2 against the oracle, median / worst: one batch {one[0]:.4f} / {one[1]:.4f} ({one[2]}), "
          f"accumulated {acc[0]:.4f} / {acc[1]:.4f} ({acc[2]})")
    assert acc[0] < REL_L2_MEDIAN and acc[1] < REL_L2_WORST, acc
    assert acc[0] <= 1.25 * one[0] and acc[1] <= 1.25 * one[1], (one, acc)
    # the single EMA of the group against the oracle's on the B = 2 statistics (tolerances: the first step of
    # tests/test_gpu_parity.py::test_multi_step_trajectory_vs_oracle - identical weights on both sides)
    K, gamma = hps.bn_vq_n_embed, hps.bn_vq_ema_gamma
    z_sum, n_sum = R.vqema_stats(out["ze"], out["min_ind"], K)
    e0 = torch.from_numpy(emb)
    numer, denom = R.vqema_ema(e0 * (1 - gamma), torch.full((K,), 1 - gamma), z_sum, n_sum, gamma)
    for nm, a, b in (("ema_numer", eng.ema_numer, numer), ("ema_denom", eng.ema_denom, denom)):
        e = float((a.cpu() - b).abs().max()) / max(float(b.abs().max()), 1e-12)
        assert e < 2e-6, (nm, e)
    assert float((eng.ema_denom.cpu() - denom).abs().max()) < 1e-6


# ----------------------------------------------------------------------------------------------
# C. MfccInverter, k = 3
# ----------------------------------------------------------------------------------------------
def test_mfcc_inverter_group_of_three():
    from ae_wavenet_amd import config, mfcc_inverter as mi, optim
    hps = config.make_hps("mi", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, n_win_batch=96, n_blocks=2,
                          n_block_layers=3, n_global_embed=4, n_speakers=5)
    torch.manual_seed(3)
    m = mi.MfccInverter(hps, accumulate=3).to(DEV)
    twin = mi.MfccInverter(hps).to(DEV)
    twin.load_state_dict(m.state_dict())
    g = m.geom
    gen = torch.Generator().manual_seed(2)
    mbs = [(torch.randint(0, 256, (2, g.enc_in_len), generator=gen).float().to(DEV),
            torch.randn(2, hps.n_lc_in, g.mel_len, generator=gen).to(DEV),
            torch.randint(0, 5, (2,), generator=gen).to(DEV), torch.arange(g.embed_len).repeat(2, 1).to(DEV)) for _ in range(3)]
    opt = optim.FusedAdam(m, lr=1e-3)
    own = []
    for j, mb in enumerate(mbs):
        twin.zero_grad()
        twin.run(*mb)[2].backward()
        n = twin._engine.ps.numel
        own.append(twin._engine.ps.grads[:n].cpu().numpy().copy())
        opt.zero_grad()
        m.run(*mb)[2].backward()
        eng = m._engine
        want = sequential_sum(own) if j == 2 else own[j]             # own gradient, own gradient, then the group's sum
        assert bits(eng.ps.grads[:n]) == want.tobytes(), j
        assert eng.step_count == 0
        opt.step()
        assert eng.step_count == (1 if j == 2 else 0)
    assert eng.acc_stats is None and (m.micro_step, m.group_ready) == (0, False)
    # the step saw the mean: a plain step of the twin on the sum with grad_scale = 1 / 3
    twin._engine.ps.grads[:n].copy_(torch.from_numpy(sequential_sum(own)))
    twin._engine.adam_step(1e-3, 1.0 / 3)
    assert bits(eng.ps.params[:n]) == bits(twin._engine.ps.params[:n])
