"""Gradient noise statistics on the GPU, through ctypes -> C ABI: AEW_OP_GRAD_WELFORD and AEW_OP_SEG_SELECT bit for bit
against the numpy restatement of tests/grad_stats_emulator.py (between canaries), and the module surface
(ae_wavenet_amd/grad_analysis.py) on the tiny models of tests/test_evaluate_gpu.py / tests/test_surface_gpu.py: grad_stats
equals the emulator applied to the gradients the closure saw, writes nothing a training step reads, leaves a training
trajectory bit-equal, does not synchronise the host, survives a change of batch size - and reproduces the quantiles the
reference's own grad_analysis.py recorded (tests/golden/grad_stats.npz)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, grad_analysis as GA
from tests import grad_stats_emulator as E
from tests.test_evaluate_gpu import _mi, _mi_batch
from tests.test_grad_stats_cpu import GOLD, TAKING_PART
from tests.test_surface_gpu import _batch, _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
CANARY = -12345.5
SIZES = [1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5, 70001]     # pads, a chunk edge on either side, many chunks, > 65535
OFFS, TOTAL = E.padded_offsets(SIZES)
CHUNKS, FIRST = L.uw_chunks(OFFS, SIZES)
NCH, P = FIRST[-1], len(SIZES)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(op):
    fail = C.c_int(-1)
    rc = L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
    torch.cuda.synchronize()
    return rc


def framed(n, dtype=torch.float32, fill=CANARY):
    """A device allocation of n elements with PAD canaries in front and behind: (whole, view)."""
    t = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    return t, t[PAD:PAD + n]


def frame_ok(whole, n):
    w = whole.cpu().numpy()
    return bool((w[:PAD] == CANARY).all() and (w[PAD + n:] == CANARY).all())


def tables():
    ch = torch.frombuffer(bytearray(bytes(CHUNKS))[:16 * NCH], dtype=torch.int64).to(DEV)
    return ch, torch.tensor(FIRST, dtype=torch.int32, device=DEV)


def same_bits(t, want):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()


# ----------------------------------------------------------------------------------------------
# 1. AEW_OP_GRAD_WELFORD
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_counts", [True, False])
def test_welford_against_the_emulator_between_canaries(reference_counts):
    rs = np.random.RandomState(7 + reference_counts)
    ch, first = tables()
    bufs = {}
    for mode in ("plain", "part"):
        bufs[mode] = dict(g=framed(TOTAL), mu=framed(TOTAL), s=framed(TOTAL))
    part_w, part = framed(2 * NCH, torch.float64)
    sums = torch.zeros(2 * P, dtype=torch.float64, device=DEV)
    mu = s = None
    for b in range(6):
        g = (rs.standard_normal(TOTAL) * 10.0 ** rs.randint(-3, 3)).astype(np.float32)
        if b == 2:
            g[:] = last                                  # a repeated sample: d is a rounding error, s barely moves
        last = g
        div = b if reference_counts else b + 1
        mu, s = E.welford(g, mu, s, b == 0, div)
        for mode in ("plain", "part"):
            B = bufs[mode]
            B["g"][1].copy_(torch.from_numpy(g))
            op = L.Op()
            op.kind = L.OP_GRAD_WELFORD
            w = op.u.gwel
            w.g, w.mu, w.s, w.n = B["g"][1].data_ptr(), B["mu"][1].data_ptr(), B["s"][1].data_ptr(), TOTAL
            w.first, w.divisor = int(b == 0), float(div)
            if mode == "part":
                w.chunks, w.chunks_host, w.n_chunks, w.part = ch.data_ptr(), C.addressof(CHUNKS), NCH, part.data_ptr()
            assert run(op) == 0
            assert same_bits(B["mu"][1], mu) and same_bits(B["s"][1], s), (b, mode)    # the pad elements included
            assert same_bits(B["g"][1], g) and all(frame_ok(B[k][0], TOTAL) for k in B), (b, mode)
        want_part = E.part_sums(mu, s, OFFS, SIZES)
        assert same_bits(part, want_part) and frame_ok(part_w, 2 * NCH), b
        op = L.Op()
        op.kind = L.OP_UPDATE_RATIO
        r = op.u.ratio
        r.part, r.first, r.n_tensors, r.finalize, r.sums = part.data_ptr(), first.data_ptr(), P, 0, sums.data_ptr()
        assert run(op) == 0
        assert same_bits(sums, E.tensor_sums(want_part, FIRST)), b
        if reference_counts and b == 1:
            assert (s < 0).any(), "the reference's count convention: mu' overshoots the sample, s goes negative"


def test_welford_scalar_tail_and_first_sample_ignore_what_mu_and_s_held():
    n = 4 * 300 + 3                                      # not a multiple of 4: the scalar tail of the plain launch
    rs = np.random.RandomState(3)
    g0, g1 = rs.standard_normal((2, n)).astype(np.float32)
    (gw, g), (mw, mu), (sw, s) = framed(n), framed(n), framed(n)
    mu.fill_(float("nan"))
    s.fill_(float("inf"))
    want = (None, None)
    for b, x in enumerate((g0, g1)):
        g.copy_(torch.from_numpy(x))
        op = L.Op()
        op.kind = L.OP_GRAD_WELFORD
        w = op.u.gwel
        w.g, w.mu, w.s, w.n, w.first, w.divisor = g.data_ptr(), mu.data_ptr(), s.data_ptr(), n, int(b == 0), 3.0
        assert run(op) == 0
        want = E.welford(x, want[0], want[1], b == 0, 3.0)
        assert same_bits(mu, want[0]) and same_bits(s, want[1])
    assert frame_ok(gw, n) and frame_ok(mw, n) and frame_ok(sw, n)


# ----------------------------------------------------------------------------------------------
# 2. AEW_OP_SEG_SELECT
# ----------------------------------------------------------------------------------------------
def select_fill():
    """The flat buffer, every tensor filled to break one pass of the radix select."""
    rs = np.random.RandomState(11)
    s = np.full(TOTAL, CANARY, np.float32)               # (the pads hold a value that must never be counted)
    u = lambda bits: np.asarray(bits, np.uint32).view(np.float32)
    fills = [
        np.float32([2.5]),                                                           # one element
        np.float32([np.nan, -1.0, -np.inf]),                                         # nothing but the NaN key
        np.float32([-0.0, 1e-42, np.inf, 0.0]),                                      # -0, a denormal, +inf
        np.full(4095, 7.25, np.float32),                                             # all elements equal
        u(0x3F800000 + rs.randint(0, 256, 4096)),                                    # differ in the lowest byte only
        u(rs.randint(0, 0x7F, 4097).astype(np.uint32) << 24 | 0x00345678),           # ... in the highest byte only
        np.concatenate([rs.rand(5000), np.full(2300, 0.5), rs.rand(4993)]).astype(np.float32),    # duplicates straddling k
        np.concatenate([np.full(40000, 3.0), rs.standard_normal(30001) * 5]).astype(np.float32)]   # 40 000 copies, negatives
    fills[6] = fills[6][rs.permutation(SIZES[6])]
    fills[7] = fills[7][rs.permutation(SIZES[7])]
    for o, n, f in zip(OFFS, SIZES, fills):
        assert f.size == n
        s[o:o + n] = f
    return s


@pytest.mark.parametrize("Q", [1, 8])
def test_select_against_the_emulator(Q):
    s_host = select_fill()
    sw, s = framed(TOTAL)
    s.copy_(torch.from_numpy(s_host))
    ch, _ = tables()
    qs = [0.5] if Q == 1 else [0, 0.1, 0.5, 0.5, 0.75, 0.9, 0.999, 1]        # two equal ranks, ranks 1 and len
    ks = np.array([E.ranks(qs, n) for n in SIZES], np.int32)
    if Q == 8:
        assert (ks[:, 0] == 1).all() and (ks[:, -1] == SIZES).all() and (ks[:, 2] == ks[:, 3]).all()
        assert 5000 < ks[6, 2] <= 7300 and ks[7, 2] > 15000                   # inside the runs of duplicates
    k = torch.from_numpy(ks).to(DEV)
    p0 = L.SegSelect()
    p0.n_tensors, p0.Q = P, Q
    nbytes = C.c_int64()
    assert L.load().aew_seg_select_size(C.byref(p0), C.byref(nbytes)) == 0
    scw, scratch = framed(nbytes.value // 4, torch.int32, fill=-777)          # (never zeroed by the caller)
    for raw, denom in ((1, 0.0), (0, 5.0), (0, 1.0)):
        want = E.seg_select(s_host, OFFS, SIZES, ks, bool(raw), denom)
        outs = []
        for call in range(2):                            # a second call on the same scratch: identical bits
            ow, out = framed(P * Q)
            op = L.Op()
            op.kind = L.OP_SEG_SELECT
            p = op.u.ssel
            p.s, p.chunks, p.n_chunks, p.n_tensors, p.Q = s.data_ptr(), ch.data_ptr(), NCH, P, Q
            p.k, p.out, p.denom, p.raw, p.scratch = k.data_ptr(), out.data_ptr(), denom, raw, scratch.data_ptr()
            assert run(op) == 0
            got = out.cpu().numpy().reshape(P, Q)
            assert frame_ok(ow, P * Q) and same_bits(s, s_host) and frame_ok(sw, TOTAL)
            w = scw.cpu().numpy()
            assert (w[:PAD] == -777).all() and (w[PAD + nbytes.value // 4:] == -777).all()
            outs.append(got.tobytes())
            for t in range(P):
                assert E.same_numbers(got[t], want[t]), (raw, denom, t, got[t], want[t])
            nan = np.isnan(want)
            assert got[~nan].tobytes() == want[~nan].tobytes()                   # bit for bit where it is a number
        assert outs[0] == outs[1]
    assert np.isnan(want[1]).all() and not np.isnan(want[3]).any()


def test_select_rank_outside_the_tensor_is_nan_not_a_fault():
    sw, s = framed(TOTAL)
    s.copy_(torch.from_numpy(select_fill()))
    ch, _ = tables()
    ks = np.array([[0, n + 1, -5] for n in SIZES], np.int32)
    k = torch.from_numpy(ks).to(DEV)
    out = torch.zeros(P * 3, device=DEV)
    scratch = torch.zeros(P * 3 * 258 + 4, dtype=torch.int32, device=DEV)
    op = L.Op()
    op.kind = L.OP_SEG_SELECT
    p = op.u.ssel
    p.s, p.chunks, p.n_chunks, p.n_tensors, p.Q = s.data_ptr(), ch.data_ptr(), NCH, P, 3
    p.k, p.out, p.denom, p.raw, p.scratch = k.data_ptr(), out.data_ptr(), 1.0, 1, scratch.data_ptr()
    assert run(op) == 0
    assert torch.isnan(out).all() and frame_ok(sw, TOTAL)


# ----------------------------------------------------------------------------------------------
# 3. - 5. the module surface
# ----------------------------------------------------------------------------------------------
QS = [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1]


def _models():
    hps, m = _mi()
    yield "mi", m, (lambda B, seed: _mi_batch(m, hps, B, seed))
    hps2, m2 = _tiny()
    yield "vqvae-ema", m2, (lambda B, seed: _batch(m2, B, seed=seed))


def _state(m):
    eng = m._engine
    torch.cuda.synchronize()
    n = eng.ps.numel
    st = dict(params=eng.ps.params[:n], grads=eng.ps.grads[:n], m=eng.adam_m[:n], v=eng.adam_v[:n])
    out = {k: v.cpu().numpy().tobytes() for k, v in st.items()}
    out["counters"] = (eng.step_count, eng.weights_version, eng.avg_steps)
    return out


def _emulate(samples, reference_counts):
    """{name: (mu, s)} of the emulator over the recorded gradient clones."""
    out = {}
    for name in samples[0]:
        mu = s = None
        for b, smp in enumerate(samples):
            mu, s = E.welford(smp[name], mu, s, b == 0, b if reference_counts else b + 1)
        out[name] = (mu, s)
    return out


@pytest.mark.parametrize("reference_counts", [True, False])
def test_grad_stats_through_the_model_equals_the_emulator_and_writes_nothing_else(reference_counts):
    from ae_wavenet_amd import optim
    for kind, m, batch in _models():
        opt = optim.FusedAdam(m, lr=1e-3)
        opt.zero_grad()
        _, _, loss = m.run(*batch(2, 1))
        loss.backward()
        opt.step()                                       # (moments and counters hold something)
        samples, calls = [], [0]

        def closure():
            opt.zero_grad()
            _, _, loss = m.run(*batch(2, 10 + calls[0]))
            loss.backward()
            if calls[0] > 0:                             # (the first call only decides who takes part)
                samples.append({n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()})
            calls[0] += 1

        closure()
        calls[0] = 0
        samples.clear()
        before = _state(m)
        res = GA.grad_stats(m, closure, 4, QS, reference_counts=reference_counts)
        after = _state(m)
        assert calls[0] == 5 and len(samples) == 4
        # the closure's own steps rewrite the gradients; everything else keeps its bits
        assert all(after[k] == before[k] for k in ("params", "m", "v", "counters")), kind
        want = _emulate(samples, reference_counts)
        assert list(res) == [n for n, _ in m.named_parameters()]
        for name, (mu, s) in want.items():
            exp = [E.kth(s, k, raw=False, denom=4) for k in E.ranks(QS, s.size)]
            assert E.same_numbers(np.float32(res[name]), np.float32(exp)), (kind, name, res[name], exp)
        # the streaming form over the same closure: state bit for bit, and add() leaves the gradients alone too
        gs = GA.GradStats(m, reference_counts=reference_counts)
        samples = []                                     # (recorded anew: a forward moves the EMA codebook)
        for b in range(4):
            opt.zero_grad()
            _, _, loss = m.run(*batch(2, 11 + b))
            loss.backward()
            samples.append({n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()})
            pre = _state(m)
            gs.add()
            assert _state(m) == pre, (kind, b)
        assert gs.count == 4
        want = _emulate(samples, reference_counts)
        for name, (mu, s) in want.items():
            assert same_bits(gs.view(name, "mu"), mu) and same_bits(gs.view(name, "s"), s), (kind, name)
        sums = gs.sums().cpu().numpy()
        names = gs.names
        for j in (0, len(names) // 2, len(names) - 1):   # the fp64 sums in the documented order (every tensor: the op test)
            mu, s = want[names[j]]
            part = E.part_sums(mu, s, [0], [s.size])
            assert sums[:, j].tobytes() == E.tensor_sums(part, [0, len(part)])[:, 0].tobytes(), (kind, names[j])
        ns = gs.noise_scale(2)
        tot = sums.sum(1)
        tr = tot[0] / 3
        assert ns.dim() == 0 and ns.dtype == torch.float64 and ns.device.type == "cuda"
        assert abs(float(ns) - 2 * tr / (tot[1] - tr / 4)) <= 1e-6 * abs(float(ns))
        gs.reset()
        assert gs.count == 0
        _, _, loss = m.run(*batch(2, 30))
        loss.backward()
        gs.add()
        assert gs.count == 1 and bool(torch.isnan(gs.noise_scale(2)))             # one sample: no variance yet


def _trajectory(with_stats):
    from ae_wavenet_amd import optim
    hps, m = _tiny()
    opt = optim.FusedAdam(m, lr=1e-3, ema_decay=0.9, max_grad_norm=1.0)
    gs = GA.GradStats(m) if with_stats else None
    batch = _batch(m, 2)
    for step in range(3):
        opt.zero_grad()
        _, _, loss = m.run(*batch)
        loss.backward()
        if gs is not None:
            gs.add()
            gs.sigma_quantiles([0.5])
        opt.step()
    torch.cuda.synchronize()
    eng = m._engine
    n = eng.ps.numel
    state = dict(params=eng.ps.params[:n], grads=eng.ps.grads[:n], m=eng.adam_m[:n], v=eng.adam_v[:n], avg=eng.adam_avg[:n],
                 emb=eng.emb, ema_numer=eng.ema_numer, ema_denom=eng.ema_denom)
    return {k: v.cpu().numpy().tobytes() for k, v in state.items()}, (eng.step_count, eng.avg_steps)


def test_training_trajectory_is_bit_equal_with_gradient_statistics_after_every_backward():
    plain, cnt_a = _trajectory(False)
    mixed, cnt_b = _trajectory(True)
    assert cnt_a == cnt_b == (3, 3)
    for k in plain:
        assert plain[k] == mixed[k], k


def test_add_and_quantiles_do_not_synchronise_the_host():
    hps, m = _tiny()
    batch = _batch(m, 2)
    gs = GA.GradStats(m)
    for _ in range(2):                                   # builds the engine, allocates the statistics and the scratch
        _, _, loss = m.run(*batch)
        loss.backward()
        gs.add()
    gs.sigma_quantiles(QS)
    gs.sums()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")              # .item() / .cpu() / a blocking copy would raise
    try:
        gs.add()
        q = gs.sigma_quantiles(QS)
        ns = gs.noise_scale(2)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert gs.count == 3 and tuple(q.shape) == (len(gs.names), len(QS)) and q.device.type == "cuda" and ns.dim() == 0


def test_statistics_survive_a_change_of_batch_size():
    hps, m = _tiny()
    gs = GA.GradStats(m)
    samples = []
    for b, B in enumerate((2, 2, 1, 1, 2)):              # a new engine at b = 2 and again at b = 4
        _, _, loss = m.run(*_batch(m, B, seed=20 + b))
        loss.backward()
        samples.append({n: p.grad.detach().cpu().numpy().reshape(-1).copy() for n, p in m.named_parameters()})
        gs.add()
    assert m._engine.B == 2 and gs.count == 5
    want = _emulate(samples, False)
    table = gs.sigma_quantiles(QS).cpu().numpy()
    for i, name in enumerate(gs.names):
        mu, s = want[name]
        assert same_bits(gs.view(name, "mu"), mu) and same_bits(gs.view(name, "s"), s), name
        exp = [E.kth(s, k, raw=False, denom=5) for k in E.ranks(QS, s.size)]
        assert E.same_numbers(table[i], np.float32(exp)), name


def test_grad_stats_reproduces_the_references_recorded_quantiles():
    """The reference's own run (tests/golden/grad_stats.npz: four parameters, one without a gradient, a NaN quantile from
    its count convention) replayed through the drop-in on a plain nn.Module."""
    shapes = {n: tuple(int(v) for v in str(sh).split(",")) for n, sh in zip(GOLD["names"], GOLD["shapes"])}

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for n, shp in shapes.items():
                setattr(self, n, torch.nn.Parameter(torch.zeros(shp)))

    model = Tiny().to(DEV)
    calls = [0]

    def closure():
        for n, p in model.named_parameters():
            p.grad = None if n == str(GOLD["no_grad"]) else torch.from_numpy(GOLD["seq_" + n][calls[0]]).reshape(shapes[n]).to(DEV)
        calls[0] += 1

    res = GA.grad_stats(model, closure, int(GOLD["n_batch"]), list(GOLD["quantiles"]))
    assert list(res) == TAKING_PART and calls[0] == 6
    for n in TAKING_PART:
        assert E.same_numbers(np.float32(res[n]), GOLD["quant_" + n]), (n, res[n], GOLD["quant_" + n])
    assert any(np.isnan(res[n]).any() for n in TAKING_PART)
