"""Global-norm gradient clipping on the GPU, through ctypes -> C ABI: the AEW_OP_GRAD_NORM op (aew_grad_norm_t), the
clip word of the Adam op (aew_adam_t.clip), the engine / FusedAdam surface and the sharded data-parallel step over RCCL.

References: numpy in fp64 for the sums; torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU for the steps."""
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

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = L.GRAD_NORM_CHUNK                      # floats per block


def stream():
    return torch.cuda.current_stream().cuda_stream


def _data(n, seed):
    """fp32 values with magnitudes spread over about 1e-4 .. 1e2"""
    rs = np.random.RandomState(seed)
    return (rs.randn(n) * 10.0 ** rs.uniform(-4, 2, n)).astype(np.float32)


class NormOp:
    """One aew_grad_norm_t over device copies of `arrays`, with its workspace."""

    def __init__(self, arrays, max_norm=1.0, grad_scale=1.0, finalize=1, add_in=None, guard=None):
        self.lib = L.load()
        self.xs = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
        g = self.g = L.GradNorm()
        for i, x in enumerate(self.xs):
            g.x[i], g.n[i] = (x.data_ptr() if x.numel() else None), x.numel()
        g.n_ranges, g.finalize = len(self.xs), finalize
        g.max_norm, g.grad_scale, g.eps = max_norm, grad_scale, 1e-6
        nd, nt = C.c_int64(), C.c_int32()
        L.check(self.lib.aew_grad_norm_size(C.byref(g), C.byref(nd), C.byref(nt)), "aew_grad_norm_size")
        assert nd.value == max(1, sum((x.numel() + CH - 1) // CH for x in self.xs)) and nt.value == 1
        self.scratch = torch.full((nd.value,), float("nan"), dtype=torch.float64, device=DEV)
        self.ticket = torch.zeros(nt.value, dtype=torch.int32, device=DEV)           # zeroed ONCE
        self.sumsq = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        self.out = torch.zeros(4, dtype=torch.float32, device=DEV)
        self.add_in = None if add_in is None else torch.tensor([add_in], dtype=torch.float64, device=DEV)
        self.guard = None if guard is None else torch.tensor([guard], dtype=torch.int32, device=DEV)
        g.sumsq, g.out, g.scratch, g.ticket = self.sumsq.data_ptr(), self.out.data_ptr(), self.scratch.data_ptr(), self.ticket.data_ptr()
        g.add_in = None if self.add_in is None else self.add_in.data_ptr()
        g.guard = None if self.guard is None else self.guard.data_ptr()

    def run(self, **over):
        for k, v in over.items():
            setattr(self.g, k, v)
        pl = Plan("norm")
        pl.add(L.OP_GRAD_NORM, self.g, "grad norm")
        pl.run(stream())
        torch.cuda.synchronize()
        return float(self.sumsq.cpu()[0]), self.out.cpu().numpy().copy()

    def rc(self):
        op = L.Op()
        op.kind = L.OP_GRAD_NORM
        op.u.gnorm = self.g
        fail = C.c_int(-1)
        rc = self.lib.aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
        torch.cuda.synchronize()
        return rc


def _coef_ref(norm, c):
    return min(1.0, c / (norm + 1e-6))


NORM_CASES = {f"n={n}": dict(arrays=[n]) for n in (1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7)}
NORM_CASES["eight ranges, one empty"] = dict(arrays=[5, CH + 3, 0, 2 * CH, 7, 4096, CH - 4, 333])
NORM_CASES["add_in"] = dict(arrays=[CH + 9, 0, 41], add_in=12345.678)
NORM_CASES["grad_scale=0.125"] = dict(arrays=[2 * CH + 7], grad_scale=0.125)


@pytest.mark.parametrize("case", list(NORM_CASES))
def test_norm_op_against_numpy_fp64(case):
    cfg = NORM_CASES[case]
    arrays = [_data(n, 10 + i) for i, n in enumerate(cfg["arrays"])]
    gs, add_in = cfg.get("grad_scale", 1.0), cfg.get("add_in")
    want_sq = sum(float(np.sum(a.astype(np.float64) ** 2)) for a in arrays) + (add_in or 0.0)
    want_norm = gs * np.sqrt(want_sq)
    op = NormOp(arrays, grad_scale=gs, add_in=add_in)
    # clipped (c = norm / 2), not clipped (c = 2 norm), and c = the fp32 norm the op itself reported: norm <= c, so the
    # coefficient is the clamp's exact 1.0 (no division)
    out = None
    for which in ("half", "double", "equal"):
        c = {"half": 0.5 * want_norm, "double": 2.0 * want_norm}.get(which) or float(out[0])
        sq, out = op.run(max_norm=c)
        # n positive terms in fp64, whatever the association: relative error <= n * 2^-53 (3.7e-12 at the largest case)
        assert abs(sq / want_sq - 1) < 1e-11, (case, sq, want_sq)
        # fp64 accumulation, one fp32 rounding of the output
        assert abs(out[0] / want_norm - 1) < 1e-6 and abs(out[0] / (gs * np.sqrt(sq)) - 1) < 1e-6, (case, out[0], want_norm)
        if which == "half":
            assert abs(out[1] / _coef_ref(want_norm, c) - 1) < 1e-6 and out[1] < 1.0, (case, c, out[1])
        else:
            assert out[1] == np.float32(1.0), (case, which, out[1])          # exactly: multiplying by it changes no bit
        assert out[2] == 0.0 and out[3] == 0.0
        assert int(op.ticket.cpu()[0]) == 0


def test_one_summation_order():
    """The same launch twice, then once more after other work on the stream: sumsq and out bit for bit, ticket back at
    zero.  Many blocks (8 ranges, 50 chunks), so the order of arrival at the ticket varies."""
    arrays = [_data(n, 40 + i) for i, n in enumerate((7 * CH + 5, 3, 9 * CH, 0, 11 * CH + 1, CH - 1, 13 * CH + 2, 8 * CH))]
    op = NormOp(arrays, max_norm=3.0)
    want_sq = sum(float(np.sum(a.astype(np.float64) ** 2)) for a in arrays)
    res = []
    for i in range(3):
        if i == 2:
            a = torch.randn(1024, 1024, device=DEV)
            (a @ a).sum().item()
            torch.zeros(1 << 22, device=DEV).add_(1.0)
        op.sumsq.fill_(-1.0); op.out[:3].fill_(-1.0)
        sq, out = op.run()
        res.append((np.float64(sq).tobytes(), out[:3].tobytes()))
        assert int(op.ticket.cpu()[0]) == 0
        assert abs(sq / want_sq - 1) < 1e-11
    assert res[0] == res[1] == res[2]


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_sets_flag_and_counts(bad):
    arrays = [_data(CH + 5, 1), _data(77, 2)]
    op = NormOp(arrays, max_norm=1.0)
    _, out = op.run()
    assert out[2] == 0.0 and out[3] == 0.0 and 0.0 < out[1] < 1.0
    finite = op.xs[-1][-1].clone()
    op.xs[-1][-1] = bad                                            # the last element of the last range (the scalar tail)
    for k in (1, 2):
        sq, out = op.run()
        assert not np.isfinite(sq)
        assert out[1] == 0.0 and out[2] == 1.0 and out[3] == float(k), out
    op.xs[-1][-1] = finite
    sq, out2 = op.run()
    assert np.isfinite(sq) and out2[2] == 0.0 and out2[3] == 2.0 and 0.0 < out2[1] < 1.0      # the count stays
    # guard word non-zero: out[] untouched
    g = NormOp(arrays, max_norm=1.0, guard=3)
    g.out.copy_(torch.tensor([9.0, 8.0, 7.0, 6.0]))
    g.run()
    assert g.out.cpu().tolist() == [9.0, 8.0, 7.0, 6.0]


def test_argument_errors():
    op = NormOp([_data(64, 1), _data(64, 2)])
    assert op.rc() == 0
    op.g.x[1] = op.xs[1].data_ptr() + 4                            # misaligned range
    assert op.rc() == L.E_ALIGN
    op.g.x[1] = op.xs[1].data_ptr()
    for nr in (0, 9, -1):
        op.g.n_ranges = nr
        assert op.rc() == L.E_ARG, nr
    op.g.n_ranges = 2
    op.g.n[0] = -1
    assert op.rc() == L.E_ARG
    op.g.n[0] = 64
    op.g.out = None                                                # finalize without out
    assert op.rc() == L.E_ARG
    op.g.finalize = 0
    assert op.rc() == 0
    nd, nt = C.c_int64(), C.c_int32()
    op.g.n_ranges = 9
    assert op.lib.aew_grad_norm_size(C.byref(op.g), C.byref(nd), C.byref(nt)) == L.E_ARG
    assert int(op.ticket.cpu()[0]) == 0


# ----------------------------------------------------------------------------------------------
# clipped Adam against clip_grad_norm_ + torch.optim.Adam on the CPU
# ----------------------------------------------------------------------------------------------
def _torch_clipped_steps(p0, grads, lr, c, betas=(0.9, 0.999), eps=1e-8):
    """[(p, m, v) after each step]: torch.nn.utils.clip_grad_norm_ then torch.optim.Adam, CPU fp32, zero initial moments."""
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    out = []
    for g in grads:
        p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p], c)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def test_clipped_adam_against_torch():
    n, lr, c, b1, b2 = 4099, 1e-3, 1.0, 0.9, 0.999                 # n % 4 = 3: the scalar tail of both kernels
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (10.0 * c / n ** 0.5) for _ in range(3)]      # norm about 10 c
    ref = _torch_clipped_steps(p0, grads, lr, c, (b1, b2))
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    g = torch.zeros(n, device=DEV)
    nop = NormOp([np.zeros(n, np.float32)], max_norm=c)
    nop.g.x[0] = g.data_ptr()
    ad = L.Adam()
    ad.p, ad.g, ad.m, ad.v, ad.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n
    ad.lr, ad.beta1, ad.beta2, ad.eps, ad.grad_scale = lr, b1, b2, 1e-8, 1.0
    ad.clip = nop.out.data_ptr() + 4

    def step(t):
        ad.bc1, ad.bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        pl = Plan("clipped adam")
        pl.add(L.OP_GRAD_NORM, nop.g, "grad norm")
        pl.add(L.OP_ADAM, ad, "adam")
        pl.run(stream())
        torch.cuda.synchronize()

    for t, gr in enumerate(grads, 1):
        g.copy_(gr)
        step(t)
        o = nop.out.cpu()
        assert abs(float(o[0]) / float(gr.double().norm()) - 1) < 1e-6 and 0.05 < float(o[1]) < 0.2 and o[2] == 0
        for got, want, what in zip((p, m, v), ref[t - 1], "pmv"):
            assert torch.allclose(got.cpu(), want, rtol=2e-6, atol=1e-7), (t, what, float((got.cpu() - want).abs().max()))
    # a step with nan in the gradient: p, m, v keep their bits
    before = [x.clone() for x in (p, m, v)]
    g.copy_(grads[0]); g[n // 2] = float("nan")
    step(4)
    assert nop.out.cpu().tolist()[1:] == [0.0, 1.0, 1.0]
    for got, was in zip((p, m, v), before):
        assert torch.equal(got, was)
    # and the next finite one moves them again
    g.copy_(grads[1])
    step(4)
    assert not torch.equal(p, before[0]) and nop.out.cpu().tolist()[2:] == [0.0, 1.0]


# ----------------------------------------------------------------------------------------------
# engine and module surface
# ----------------------------------------------------------------------------------------------
def _two_steps(mode, lr=1e-3):
    from ae_wavenet_amd import optim
    from tests.test_surface_gpu import _batch, _tiny
    hps, m = _tiny()
    batch = _batch(m, 2)
    opt = optim.FusedAdam(m, lr=lr, max_grad_norm=1e30 if mode == "huge" else None)
    for _ in range(2):
        opt.zero_grad()
        _, _, loss = m.run(*batch)
        loss.backward()
        if mode == "null":                                         # the engine's own default path: the descriptor has no clip word
            m._engine.adam_step(lr)
            assert not m._engine.opt.array()[0].u.adam.clip
        else:
            opt.step()
    torch.cuda.synchronize()
    eng = m._engine
    n = eng.ps.numel
    assert bool(eng.opt.array()[0].u.adam.clip) == (mode == "huge")
    if mode == "huge":
        o = eng.grad_norm().cpu()
        assert o[0] > 0 and o[1] == 1.0 and o[2] == 0 and o[3] == 0
    return eng.ps.params[:n].clone(), eng.adam_m[:n].clone(), eng.adam_v[:n].clone()


def test_off_means_off():
    """max_grad_norm=None, max_grad_norm=1e30 (coefficient exactly 1.0) and the engine step without the argument
    (clip = NULL): parameters and both moments bit for bit after two steps on a fixed batch."""
    a, b, c = _two_steps("none"), _two_steps("huge"), _two_steps("null")
    for x, y, z, what in zip(a, b, c, ("params", "m", "v")):
        assert torch.equal(x, y), (what, "max_grad_norm=1e30")
        assert torch.equal(x, z), (what, "clip=NULL")


def test_fused_adam_surface_clips_like_clip_grad_norm():
    from ae_wavenet_amd import optim
    from tests.test_surface_gpu import _batch, _tiny
    hps, m = _tiny()
    lr = 1e-3
    _, _, loss = m.run(*_batch(m, 2))
    loss.backward()
    torch.cuda.synchronize()
    names = [n for n, _ in m.named_parameters()]
    before = [p.detach().cpu().clone() for p in m.parameters()]
    grads = [p.grad.detach().cpu().clone() for p in m.parameters()]
    # the PER-PARAMETER norm (no pad slots): what clip_grad_norm_ would see
    norm = float(torch.linalg.vector_norm(torch.cat([g.reshape(-1) for g in grads]), dtype=torch.float64))
    c = 0.5 * norm                                                 # below the first step's norm: the clip is active
    opt = optim.FusedAdam(m, lr, max_grad_norm=c)
    assert opt.param_groups[0]["max_grad_norm"] == c
    opt.step()
    torch.cuda.synchronize()
    assert opt.grad_norm.ndim == 0 and opt.grad_norm.is_cuda
    assert abs(float(opt.grad_norm) / norm - 1) < 1e-6, (float(opt.grad_norm), norm)   # pins the zero pads of the flat buffer
    assert abs(float(opt.clip_coef) / (c / (norm + 1e-6)) - 1) < 1e-6 and float(opt.clip_coef) < 1.0
    assert float(opt.skipped_steps) == 0.0
    ref = [torch.nn.Parameter(b.clone()) for b in before]
    topt = torch.optim.Adam(ref, lr=lr)
    for r, g in zip(ref, grads):
        r.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ref, c)
    topt.step()
    for nme, p, r in zip(names, m.parameters(), ref):
        assert torch.allclose(p.detach().cpu(), r.detach(), rtol=2e-6, atol=1e-7), (nme, float((p.detach().cpu() - r.detach()).abs().max()))


def test_sharded_step_with_clipping_over_rccl_on_one_rank():
    """RCCL ("nccl"), one rank, DataParallel(force_collectives=True): the sharded optimizer_step with clipping - shard
    launch, all-reduce of the fp64 word, finalizing launch with add_in over the (empty) remainders - gives the parameters
    and moments of the engine path with clipping, bit for bit.  tools/dp_rccl_clip_one_rank.py runs it in a fresh process."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dp_rccl_clip_one_rank.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    out = json.loads(lines[-1])
    assert out["backend"] == "nccl" and out["world"] == 1
    assert out["collectives"]["all_reduce_f64"] == out["steps"]          # the collective carried the fp64 word, once per step
    assert out["norm_launches"]["sharded"] == 2 * out["steps"] and out["norm_launches"]["engine"] == out["steps"]
    assert all(0.0 < w[1] < 1.0 and w[2] == 0.0 for w in out["clip_words"]["engine"]), out["clip_words"]
    assert out["clip_words"]["sharded"] == out["clip_words"]["engine"]
    assert out["bit_equal"] == {"params": True, "m": True, "v": True}, out["max_abs_diff"]
