"""Per-parameter update / weight ratios on the GPU, through ctypes -> C ABI: the tracked Adam launch (aew_adam_t.track),
the AEW_OP_UPDATE_RATIO op (aew_update_ratio_t), the engine / FusedAdam surface and the sharded data-parallel step over
RCCL.

References: numpy in fp64 over the parameters read back before and after the step (the difference taken in fp32, as the
kernel and the reference's `c - p` take it); the harness's own clone-and-norm loop for the surface."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Plan
from tests.test_update_ratio_cpu import SIZES, padded_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = L.UW_CHUNK
OFFS, TOTAL = padded_offsets(SIZES)
N = OFFS[-1] + SIZES[-1]                    # the buffer ends with the last tensor: N % 4 = 3, the scalar tail of the kernels
P = len(SIZES)


def stream():
    return torch.cuda.current_stream().cuda_stream


class Flat:
    """A synthetic flat buffer (SIZES at padded offsets, random p / g / m / v, pads included), its chunk table and the
    workspace of both ops."""

    def __init__(self, seed=0, clip=None, guard=None):
        self.lib = L.load()
        gen = torch.Generator().manual_seed(seed)
        self.state0 = [torch.randn(TOTAL, generator=gen), torch.randn(TOTAL, generator=gen) * 0.1,
                       torch.randn(TOTAL, generator=gen) * 0.01, torch.rand(TOTAL, generator=gen) * 1e-3]
        self.p, self.g, self.m, self.v = (t.to(DEV) for t in self.state0)
        self.chunks_host, self.first_host = L.uw_chunks(OFFS, SIZES)
        self.nch = self.first_host[-1]
        raw = bytearray(bytes(self.chunks_host))[:16 * self.nch]
        self.chunks = torch.frombuffer(raw, dtype=torch.int64).to(DEV)
        self.first = torch.tensor(self.first_host, dtype=torch.int32, device=DEV)
        self.part = torch.full((2 * self.nch,), float("nan"), dtype=torch.float64, device=DEV)    # the first launch clears it
        self.sums = torch.full((2 * P,), -1.0, dtype=torch.float64, device=DEV)
        self.out = torch.full((3 * P,), -1.0, dtype=torch.float32, device=DEV)
        self.clip = None if clip is None else torch.tensor(clip, dtype=torch.float32, device=DEV)
        self.guard = None if guard is None else torch.tensor([guard], dtype=torch.int32, device=DEV)
        tr = self.tr = L.UwTrack()
        tr.chunks, tr.chunks_host, tr.n_chunks = self.chunks.data_ptr(), C.addressof(self.chunks_host), self.nch
        tr.part = self.part.data_ptr()

    def reset(self):
        for t, s in zip((self.p, self.g, self.m, self.v), self.state0):
            t.copy_(s)

    def adam_rec(self, lo=0, hi=N, zero=True, track=True, t=1):
        a = L.Adam()
        a.p, a.g, a.m, a.v = (x.data_ptr() + 4 * lo for x in (self.p, self.g, self.m, self.v))
        a.n = hi - lo
        a.lr, a.beta1, a.beta2, a.eps, a.grad_scale = 1e-3, 0.9, 0.999, 1e-8, 0.5
        a.bc1, a.bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
        a.clip = None if self.clip is None else self.clip.data_ptr()
        a.guard = None if self.guard is None else self.guard.data_ptr()
        if track:
            self.tr.base, self.tr.zero = lo, int(zero)
            a.track = C.addressof(self.tr)
        return a

    def adam(self, **kw):
        pl = Plan("adam")
        pl.add(L.OP_ADAM, self.adam_rec(**kw), "adam")
        pl.run(stream())
        torch.cuda.synchronize()

    def ratio_rec(self, finalize=1, add_in=None, part=True):
        r = L.UpdateRatio()
        r.part, r.first, r.n_tensors, r.finalize = (self.part.data_ptr() if part else None), self.first.data_ptr(), P, finalize
        r.add_in = None if add_in is None else add_in.data_ptr()
        r.sums, r.out = self.sums.data_ptr(), self.out.data_ptr()
        return r

    def ratio(self, **kw):
        pl = Plan("ratio")
        pl.add(L.OP_UPDATE_RATIO, self.ratio_rec(**kw), "update ratio")
        pl.run(stream())
        torch.cuda.synchronize()
        return self.sums.cpu().numpy().reshape(2, P).copy(), self.out.cpu().numpy().reshape(3, P).copy()

    def rc(self, kind, rec):
        op = L.Op()
        op.kind = kind
        setattr(op.u, L.OP_FIELD[kind], rec)
        fail = C.c_int(-1)
        rc = self.lib.aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
        torch.cuda.synchronize()
        return rc


def _ref_sums(old, new):
    """[2][P] in fp64 from the parameters before / after: the difference in fp32, squares and sums in fp64."""
    o, n = old.cpu().numpy(), new.cpu().numpy()
    out = np.zeros((2, P))
    for t, (off, k) in enumerate(zip(OFFS, SIZES)):
        d = (o[off:off + k] - n[off:off + k]).astype(np.float64)
        out[0, t] = np.sum(d * d)
        out[1, t] = np.sum(o[off:off + k].astype(np.float64) ** 2)
    return out


def _ulps(got, want64):
    want = np.float32(want64)
    return np.abs(got.astype(np.float64) - np.float64(want)) / np.spacing(np.abs(want)).astype(np.float64)


def test_sums_and_outputs_against_numpy_fp64():
    f = Flat(1)
    old = f.p.clone()
    f.adam()
    want = _ref_sums(old, f.p)
    assert (want > 0).all()
    sums, _ = f.ratio(finalize=0)
    # identical inputs, only the summation order differs: n positive terms in fp64, relative error <= n * 2^-53
    # (n <= 2e4: 2e-12)
    assert np.abs(sums / want - 1).max() < 1e-11, np.abs(sums / want - 1).max()
    assert (f.out.cpu().numpy() == -1.0).all()                      # finalize = 0 writes the pairs only
    add = torch.tensor(np.stack([np.arange(1, P + 1) * 1e-5, np.arange(1, P + 1) * 2.0]).reshape(-1), device=DEV)
    for add_in in (None, add):
        f.sums.fill_(-1.0)
        sums1, out = f.ratio(finalize=1, add_in=add_in)
        tot = want + (0.0 if add_in is None else add_in.cpu().numpy().reshape(2, P))
        assert np.abs(sums1 / tot - 1).max() < 1e-11
        un, wn = np.sqrt(tot[0]), np.sqrt(tot[1])
        # the square root of an fp64 sum good to 1e-11, one fp32 rounding each, one correctly rounded fp32 division
        assert _ulps(out[0], un).max() <= 2 and _ulps(out[1], wn).max() <= 2 and _ulps(out[2], un / wn).max() <= 2, \
            (_ulps(out[0], un).max(), _ulps(out[1], wn).max(), _ulps(out[2], un / wn).max())
    # the sharded form's second launch: no chunk sums, the totals are add_in alone
    _, out = f.ratio(finalize=1, add_in=add, part=False)
    a = add.cpu().numpy().reshape(2, P)
    assert _ulps(out[0], np.sqrt(a[0])).max() <= 2 and _ulps(out[1], np.sqrt(a[1])).max() <= 2


def test_range_calls_equal_one_call_and_repeat_bit_for_bit():
    cut1 = OFFS[3] + 2000                                           # in the middle of a chunk
    cut2 = OFFS[5] + CH                                             # in the middle of a tensor, between two of its chunks
    cut3 = OFFS[5] + CH + 1028                                      # in the middle of a tensor AND of a chunk
    assert cut1 % 4 == 0 and cut2 % 4 == 0 and cut3 % 4 == 0 and 0 < cut1 < cut2 < cut3 < N
    f = Flat(2)
    f.adam()
    one, _ = f.ratio(finalize=0)
    p_one = f.p.clone()
    res = []
    for rep in range(2):
        f.reset()
        f.part.fill_(float("nan"))
        f.adam(lo=cut3, hi=N, zero=True)                            # the order of a data-parallel step: tail first
        f.adam(lo=cut1, hi=cut3, zero=False)
        f.adam(lo=0, hi=cut1, zero=False)
        sums, out = f.ratio(finalize=0)
        res.append((sums.tobytes(), f.part.cpu().numpy().tobytes()))
        assert torch.equal(f.p, p_one)
        assert np.abs(sums / one - 1).max() < 1e-12, np.abs(sums / one - 1).max()
    assert res[0] == res[1]
    # a cut at a chunk boundary inside a tensor
    f.reset()
    f.adam(lo=cut2, hi=N, zero=True)
    f.adam(lo=0, hi=cut2, zero=False)
    sums, _ = f.ratio(finalize=0)
    assert torch.equal(f.p, p_one) and np.abs(sums / one - 1).max() < 1e-12


@pytest.mark.parametrize("clip", [None, [0.37, 0.0]])
def test_tracked_step_leaves_the_bits_of_an_untracked_step(clip):
    a, b = Flat(3, clip=clip), Flat(3, clip=clip)
    for t in (1, 2):
        a.adam(track=False, t=t)
        b.adam(track=True, t=t)
        for x, y, what in zip((a.p, a.m, a.v), (b.p, b.m, b.v), "pmv"):
            assert torch.equal(x, y), (t, what, clip)               # the pad elements included
    assert not torch.equal(a.p.cpu(), a.state0[0])
    # and in range calls
    c = Flat(3, clip=clip)
    for t in (1, 2):
        c.adam(lo=OFFS[4] + 8, hi=N, t=t)
        c.adam(lo=0, hi=OFFS[4] + 8, zero=False, t=t)
    for x, y, what in zip((a.p, a.m, a.v), (c.p, c.m, c.v), "pmv"):
        assert torch.equal(x, y), (what, clip)


@pytest.mark.parametrize("how", ["clip flag", "guard word"])
def test_skipped_step_at_op_level_reports_zero_update_and_true_weight_norm(how):
    f = Flat(4, clip=[1.0, 1.0]) if how == "clip flag" else Flat(4, guard=3)
    old = [x.clone() for x in (f.p, f.m, f.v)]
    f.adam()
    for x, y in zip((f.p, f.m, f.v), old):
        assert torch.equal(x, y)
    sums, out = f.ratio()
    want = _ref_sums(old[0], old[0])
    assert (sums[0] == 0.0).all() and (out[0] == 0.0).all() and (out[2] == 0.0).all()
    assert np.abs(sums[1] / want[1] - 1).max() < 1e-11 and _ulps(out[1], np.sqrt(want[1])).max() <= 2


def test_zero_tensor_gives_the_non_finite_class_of_the_torch_expression():
    f = Flat(5)
    f.state0[0][OFFS[2]:OFFS[2] + SIZES[2]] = 0.0                   # a zero-initialised bias
    f.reset()
    old = f.p.clone()
    f.adam()
    _, out = f.ratio()
    c, p = old[OFFS[2]:OFFS[2] + SIZES[2]], f.p[OFFS[2]:OFFS[2] + SIZES[2]]
    ref = float(torch.norm(c - p) / c.norm())
    assert np.isinf(ref) and np.isinf(out[2, 2]) and out[2, 2] > 0 and out[1, 2] == 0.0 and out[0, 2] > 0
    assert np.isfinite(np.delete(out[2], 2)).all()
    # the tensor did not move either (a skipped step): 0 / 0
    g = Flat(5, clip=[1.0, 1.0])
    g.state0[0][OFFS[2]:OFFS[2] + SIZES[2]] = 0.0
    g.reset()
    g.adam()
    _, out = g.ratio()
    c = g.p[OFFS[2]:OFFS[2] + SIZES[2]]
    ref = float(torch.norm(c - c) / c.norm())
    assert np.isnan(ref) and np.isnan(out[2, 2])


def test_argument_errors():
    f = Flat(6)
    f.adam()
    ok = f.ratio_rec()
    assert f.rc(L.OP_UPDATE_RATIO, ok) == 0
    for field, val, want in (("n_tensors", 0, L.E_ARG), ("n_tensors", -1, L.E_ARG), ("first", None, L.E_ARG),
                             ("out", None, L.E_ARG), ("part", None, L.E_ARG),
                             ("part", f.part.data_ptr() + 4, L.E_ALIGN), ("sums", f.sums.data_ptr() + 4, L.E_ALIGN),
                             ("out", f.out.data_ptr() + 2, L.E_ALIGN), ("first", f.first.data_ptr() + 2, L.E_ALIGN)):
        r = f.ratio_rec()
        setattr(r, field, val)
        assert f.rc(L.OP_UPDATE_RATIO, r) == want, (field, val)
    r = f.ratio_rec(finalize=0)
    r.sums = None
    assert f.rc(L.OP_UPDATE_RATIO, r) == L.E_ARG                    # finalize = 0 has nothing else to write
    r = f.ratio_rec(finalize=0, part=False, add_in=f.sums)
    assert f.rc(L.OP_UPDATE_RATIO, r) == L.E_ARG                    # ... and nothing to reduce without the chunk sums
    r = f.ratio_rec(finalize=1, part=False, add_in=f.sums)
    r.sums = None
    assert f.rc(L.OP_UPDATE_RATIO, r) == 0                          # the sharded form's second launch
    # the tracking record of the Adam op: every refusal comes before any launch
    before = [x.clone() for x in (f.p, f.m, f.v)]
    for field, val, want in (("chunks", None, L.E_ARG), ("chunks_host", None, L.E_ARG), ("part", None, L.E_ARG),
                             ("n_chunks", 0, L.E_ARG), ("base", -4, L.E_ARG), ("base", 2, L.E_ALIGN),
                             ("part", f.part.data_ptr() + 8, L.E_ALIGN),
                             ("base", TOTAL, L.E_ARG),              # the range lies behind every chunk
                             ("n_chunks", 3, L.E_ARG)):             # the table ends in front of the range's end
        a = f.adam_rec()
        keep = getattr(f.tr, field)
        setattr(f.tr, field, val)
        rc = f.rc(L.OP_ADAM, a)
        setattr(f.tr, field, keep)
        assert rc == want, (field, val, rc)
    a = f.adam_rec()
    a.n = 0
    assert f.rc(L.OP_ADAM, a) == L.E_ARG
    for x, y in zip((f.p, f.m, f.v), before):
        assert torch.equal(x, y)
    assert f.rc(L.OP_ADAM, f.adam_rec()) == 0


# ----------------------------------------------------------------------------------------------
# engine and module surface
# ----------------------------------------------------------------------------------------------
def test_skipped_step_under_max_grad_norm_with_an_inf_gradient():
    from ae_wavenet_amd import optim
    from tests.test_surface_gpu import _batch, _tiny
    hps, m = _tiny()
    opt = optim.FusedAdam(m, 1e-3, max_grad_norm=1.0, track_update_ratio=True)
    _, _, loss = m.run(*_batch(m, 2))
    loss.backward()
    eng = m._engine
    n = eng.ps.numel
    eng.ps.grads[n // 2] = float("inf")
    before = [x[:n].clone() for x in (eng.ps.params, eng.adam_m, eng.adam_v)]
    copies = {k: p.detach().double().clone() for k, p in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.skipped_steps) == 1.0
    for x, y in zip((eng.ps.params, eng.adam_m, eng.adam_v), before):
        assert torch.equal(x[:n], y)
    un, wn = opt.update_norm, opt.weight_norm
    assert list(un) == [k for k, _ in m.named_parameters()]
    moved = 0
    for k, c in copies.items():
        assert float(un[k]) == 0.0, k
        ref = float(c.norm())
        if ref > 0:
            assert abs(float(wn[k]) / ref - 1) < 1e-6, (k, float(wn[k]), ref)
            moved += 1
        else:
            assert float(wn[k]) == 0.0
    assert moved > len(copies) // 2
    # the next finite step moves the tensors again
    opt.zero_grad()
    _, _, loss = m.run(*_batch(m, 2))
    loss.backward()
    opt.step()
    assert sum(float(v) > 0 for v in opt.update_norm.values()) > len(copies) // 2


@pytest.mark.parametrize("clip", [None, 0.05])
def test_surface_against_the_harness_loop_in_the_same_step(clip):
    """tests/test_harness_gpu.py's tiny configuration, three steps: chassis.py:162-163,180-183 as written, run around
    the very step that tracks - once with torch's fp32 norms (printed and held to 1e-5) and once in fp64, which decides
    (1e-6: fp64 sums, then the fp32 roundings of two norms and one division, 6e-8 each)."""
    from ae_wavenet_amd import autoencoder_model as ae, config, optim
    hps = config.make_hps("vqvae-ema", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64, bn_n_out=16,
                          n_win_batch=256, n_blocks=2, n_block_layers=5, bn_vq_n_embed=128)
    B = 4
    torch.manual_seed(31)
    model = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    ss_optim = optim.FusedAdam(model, lr=1e-3, max_grad_norm=clip, track_update_ratio=True)
    g = model.geom
    gen = torch.Generator().manual_seed(32)
    for step in range(3):
        wav = torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(DEV)
        mel = torch.randn(B, 39, g.mel_len, generator=gen).to(DEV)
        voice = torch.randint(0, 40, (B,), generator=gen).to(DEV)
        jitter = torch.arange(g.embed_len).repeat(B, 1).to(DEV)
        ss_optim.zero_grad()
        quant, target, loss = model.run(wav, mel, voice, jitter)
        loss.backward()
        pars_copy = [p.data.clone() for p in model.parameters()]
        ss_optim.step()
        uw_ratio = {np_[0]: torch.norm(c - np_[1].data) / c.norm() for c, np_ in zip(pars_copy, model.named_parameters())}
        uw64 = {np_[0]: (c.double() - np_[1].data.double()).norm() / c.double().norm()
                for c, np_ in zip(pars_copy, model.named_parameters())}
        got = ss_optim.update_ratio
        assert list(got) == list(uw_ratio)
        e32, e64, nonfinite = 0.0, 0.0, 0
        for k in got:
            a, b32, b64 = float(got[k]), float(uw_ratio[k]), float(uw64[k])
            assert got[k].ndim == 0 and got[k].is_cuda
            if np.isfinite(b64):
                e32, e64 = max(e32, abs(a / b32 - 1)), max(e64, abs(a / b64 - 1))
            else:
                nonfinite += 1
                assert (np.isinf(a) and np.isinf(b64)) or (np.isnan(a) and np.isnan(b64)), (k, a, b64)
        print(f"clip {clip} step {step}: max relative error against torch fp32 norms {e32:.2e}, against fp64 {e64:.2e}; "
              f"{nonfinite} tensors with a zero weight norm")
        assert e32 < 1e-5, (step, e32)
        assert e64 < 1e-6, (step, e64)
        assert nonfinite < len(got) // 2
    if clip is not None:
        assert 0.0 < float(ss_optim.clip_coef) < 1.0


def test_sharded_step_over_rccl_on_one_rank():
    """RCCL ("nccl"), one rank, DataParallel(force_collectives=True): the sharded optimizer_step with tracking - shard
    calls with the record, remainder calls on rank 0, finalize = 0, the all-reduce of the 2 P fp64 words, finalize = 1
    from those words - against the unsharded engine.  tests/update_ratio_rccl_one_rank.py runs it in a fresh process."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "update_ratio_rccl_one_rank.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    out = json.loads(lines[-1])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["collectives"]["all_reduce_2P_f64"] == out["steps"]       # the collective carried the 2 P words, once per step
    assert out["ratio_launches"] == {"sharded": 2 * out["steps"], "engine": out["steps"]}
    assert out["tensors"] > 20 and out["finite"] > out["tensors"] // 2
    assert out["max_rel"]["update_norm"] < 1e-6 and out["max_rel"]["weight_norm"] < 1e-6 and out["max_rel"]["ratio"] < 1e-6, out
    assert out["same_class"] and out["bit_equal"] == {"params": True, "m": True, "v": True}, out
