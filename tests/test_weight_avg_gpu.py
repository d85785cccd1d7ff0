"""Averaged (EMA) weights on the GPU, through ctypes -> C ABI: the Adam launches with aew_adam_t.avg (untracked and
tracked, clipped and not), the AEW_OP_SWAP op (aew_swap_t), and the engine / FusedAdam surface: the average against a
numpy fp32 recursion, the swap around forward / sampling / state_dict, and the carry across engine rebuilds."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from tests.test_update_ratio_cpu import SIZES, padded_offsets
from tests.test_update_ratio_gpu import Flat, stream
from tests.weight_avg_emulator import avg_update

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = L.UW_CHUNK
OFFS, TOTAL = padded_offsets(SIZES)
N = OFFS[-1] + SIZES[-1]                    # N % 4 = 3: the scalar tail of the kernels runs
RATES = (1.0, 0.0, float(np.float32(1 - 0.999)))
CANARY = -12345.5


class AvgFlat(Flat):
    """The synthetic flat buffer of tests/test_update_ratio_gpu.py with an average beside it: random values over the
    launch's elements, canaries in front of it and behind it."""

    def __init__(self, seed=0, **kw):
        super().__init__(seed, **kw)
        gen = torch.Generator().manual_seed(seed + 1000)
        self.avg0 = torch.randn(TOTAL, generator=gen)
        self.avg0[N:] = CANARY
        self.avg_buf = torch.full((TOTAL + 8,), CANARY, device=DEV)
        self.avg = self.avg_buf[4:4 + TOTAL]                        # 16 bytes into the allocation: still aligned
        self.avg.copy_(self.avg0)

    def reset(self):
        super().reset()
        self.avg_buf.fill_(CANARY)
        self.avg.copy_(self.avg0)

    def adam_rec(self, lo=0, hi=N, zero=True, track=True, t=1, rate=None):
        a = super().adam_rec(lo=lo, hi=hi, zero=zero, track=track, t=t)
        if rate is not None:
            a.avg, a.avg_rate = self.avg.data_ptr() + 4 * lo, rate
        return a

    def canaries_intact(self):
        b = self.avg_buf.cpu().numpy()
        return (b[:4] == CANARY).all() and (b[4 + N:] == CANARY).all()


def bits(t):
    return t.detach().cpu().numpy().tobytes()


# ----------------------------------------------------------------------------------------------
# the Adam launches with an average
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("clip", [None, [0.37, 0.0]])
def test_averaged_launch_against_the_launch_without_it(clip, track):
    """All four kernel instantiations: p / m / v (and the tracked launch's chunk sums) keep the bits of the launch without
    an average; the average is the numpy fp32 restatement over the parameters read back, pads included."""
    for rate in RATES:
        a, b = AvgFlat(3, clip=clip), AvgFlat(3, clip=clip)
        want = b.avg0.numpy().copy()
        for t in (1, 2):
            a.adam(track=track, t=t)
            b.adam(track=track, t=t, rate=rate)
            for x, y, what in zip((a.p, a.m, a.v), (b.p, b.m, b.v), "pmv"):
                assert torch.equal(x, y), (rate, t, what)
            if track:
                assert bits(a.part) == bits(b.part), (rate, t)
            want[:N] = avg_update(want[:N], rate, b.p.cpu().numpy()[:N])
            assert bits(b.avg) == want.tobytes(), (rate, t, np.flatnonzero(b.avg.cpu().numpy() != want)[:8])
        assert b.canaries_intact() and bits(a.avg) == a.avg0.numpy().tobytes()     # (no average: the buffer is not touched)
        assert not torch.equal(b.p.cpu(), b.state0[0])
        if rate == 0.0:
            assert bits(b.avg) == b.avg0.numpy().tobytes()
        else:
            assert not np.array_equal(b.avg.cpu().numpy()[:N], b.avg0.numpy()[:N])
            pad = OFFS[1] + SIZES[1]                                 # a pad element behind the tensor of one element
            assert float(b.avg[pad]) != float(b.avg0[pad])


@pytest.mark.parametrize("track", [False, True])
def test_range_calls_average_exactly_their_range(track):
    cut1 = OFFS[3] + 2000                                           # inside a tensor and a chunk
    cut3 = OFFS[5] + CH + 1028
    assert cut1 % 4 == 0 and cut3 % 4 == 0 and 0 < cut1 < cut3 < N
    rate = RATES[2]
    f = AvgFlat(2)
    f.adam(track=track, rate=rate)
    one = bits(f.avg)
    f.reset()
    f.adam(lo=cut3, hi=N, zero=True, track=track, rate=rate)        # the order of a data-parallel step: tail first
    f.adam(lo=cut1, hi=cut3, zero=False, track=track, rate=rate)
    f.adam(lo=0, hi=cut1, zero=False, track=track, rate=rate)
    assert bits(f.avg) == one and f.canaries_intact()
    # one range alone: the elements outside it keep their bits
    f.reset()
    f.avg[:cut1] = CANARY
    f.avg[cut3:] = CANARY
    f.adam(lo=cut1, hi=cut3, track=track, rate=rate)
    got = f.avg.cpu().numpy()
    assert (got[:cut1] == CANARY).all() and (got[cut3:] == CANARY).all() and f.canaries_intact()
    assert got[cut1:cut3].tobytes() == np.frombuffer(one, np.float32)[cut1:cut3].tobytes()


@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("how", ["guard word", "clip flag"])
def test_skipped_step_leaves_the_average_alone(how, track):
    f = AvgFlat(4, guard=1) if how == "guard word" else AvgFlat(4, clip=[0.5, 1.0])
    old = [bits(x) for x in (f.avg_buf, f.p, f.m, f.v)]
    f.adam(track=track, rate=0.25)
    assert [bits(x) for x in (f.avg_buf, f.p, f.m, f.v)] == old


@pytest.mark.parametrize("track", [False, True])
def test_argument_errors_of_the_averaged_launch(track):
    f = AvgFlat(6)
    old = [bits(x) for x in (f.avg_buf, f.p, f.m, f.v)]
    a = f.adam_rec(track=track, rate=0.5)
    a.avg = f.avg.data_ptr() + 4
    assert f.rc(L.OP_ADAM, a) == L.E_ALIGN
    for bad in (1.5, -0.1, float("nan")):
        assert f.rc(L.OP_ADAM, f.adam_rec(track=track, rate=bad)) == L.E_ARG, bad
    assert [bits(x) for x in (f.avg_buf, f.p, f.m, f.v)] == old     # every refusal comes before any launch
    a = f.adam_rec(track=track)                                     # without an average the rate is not looked at
    a.avg_rate = 1.5
    assert f.rc(L.OP_ADAM, a) == 0
    assert f.rc(L.OP_ADAM, f.adam_rec(track=track, rate=1.0)) == 0


# ----------------------------------------------------------------------------------------------
# AEW_OP_SWAP
# ----------------------------------------------------------------------------------------------
def _swap_rc(lib, a, b, n):
    op = L.Op()
    op.kind = L.OP_SWAP
    op.u.swap.a, op.u.swap.b, op.u.swap.n = a, b, n
    fail = C.c_int(-1)
    rc = lib.aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, N])
def test_swap_exchanges_exactly_and_twice_restores(n):
    lib = L.load()
    gen = torch.Generator().manual_seed(n)
    x0, y0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    bufs = [torch.full((n + 12,), CANARY, device=DEV) for _ in range(2)]
    xa, xb = bufs[0][4:4 + n], bufs[1][4:4 + n]
    xa.copy_(x0); xb.copy_(y0)
    assert _swap_rc(lib, xa.data_ptr(), xb.data_ptr(), n) == 0
    assert bits(xa) == y0.numpy().tobytes() and bits(xb) == x0.numpy().tobytes()
    for b in bufs:
        c = b.cpu().numpy()
        assert (c[:4] == CANARY).all() and (c[4 + n:] == CANARY).all()
    assert _swap_rc(lib, xa.data_ptr(), xb.data_ptr(), n) == 0
    assert bits(xa) == x0.numpy().tobytes() and bits(xb) == y0.numpy().tobytes()
    for b in bufs:
        c = b.cpu().numpy()
        assert (c[:4] == CANARY).all() and (c[4 + n:] == CANARY).all()


def test_swap_argument_errors():
    lib = L.load()
    a, b = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    assert _swap_rc(lib, a.data_ptr() + 4, b.data_ptr(), 8) == L.E_ALIGN
    assert _swap_rc(lib, a.data_ptr(), b.data_ptr() + 8, 8) == L.E_ALIGN
    assert _swap_rc(lib, a.data_ptr(), b.data_ptr(), -1) == L.E_ARG
    assert _swap_rc(lib, None, b.data_ptr(), 8) == L.E_ARG
    assert _swap_rc(lib, a.data_ptr(), a.data_ptr() + 16, 8) == L.E_ARG      # overlapping: not an exchange
    assert _swap_rc(lib, a.data_ptr(), b.data_ptr(), 0) == 0
    assert float(a.min()) == 1.0 and float(b.max()) == 0.0


# ----------------------------------------------------------------------------------------------
# engine and module surface (the MFCC inverter configuration and batch of tests/test_surface_gpu.py)
# ----------------------------------------------------------------------------------------------
DECAY = 0.9


def _mi():
    from ae_wavenet_amd import config, mfcc_inverter as mi
    hps = config.make_hps("mi", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, n_win_batch=96, n_blocks=2,
                          n_block_layers=3, n_global_embed=4, n_speakers=5)
    torch.manual_seed(3)
    m = mi.MfccInverter(hps).to(DEV)
    g = m.geom
    gen = torch.Generator().manual_seed(2)
    batch = (torch.randint(0, 256, (2, g.enc_in_len), generator=gen).float().to(DEV),
             torch.randn(2, hps.n_lc_in, g.mel_len, generator=gen).to(DEV),
             torch.randint(0, 5, (2,), generator=gen).to(DEV), torch.arange(g.embed_len).repeat(2, 1).to(DEV))
    return hps, m, batch


def _step(m, opt, batch):
    opt.zero_grad()
    _, _, loss = m.run(*batch)
    loss.backward()
    opt.step()


def _params(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.named_parameters()}


def _avg(m, opt):
    sd = opt.state_dict()
    return {k: sd["state"][i]["param_avg"].numpy().copy() for i, (k, _) in enumerate(m.named_parameters())}


def _same(a, b):
    return list(a) == list(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def _trained(twins=1):
    """`twins` identically built models after the same three averaged steps (each test trains its own: they change
    them); the first one's average as the numpy recursion over its parameters read back after each step."""
    from ae_wavenet_amd import optim
    out, want = [], None
    for twin in range(twins):
        hps, m, batch = _mi()
        opt = optim.FusedAdam(m, lr=1e-3, ema_decay=DECAY)
        if twin == 0:
            want = _params(m)                                       # the average starts from the weights in front of step 1
        for t in range(3):
            _step(m, opt, batch)
            if twin == 0:
                new = _params(m)
                want = {k: avg_update(want[k], optim.ema_rate_at(DECAY, t), new[k]) for k in want}
        out += [m, opt]
    return dict(hps=hps, batch=batch, m=out[0], opt=out[1], m2=out[-2], opt2=out[-1], want=want)


@pytest.fixture
def trained():
    return _trained()


def test_surface_average_is_the_numpy_recursion(trained):
    m, opt = trained["m"], trained["opt"]
    got = _avg(m, opt)
    assert _same(got, trained["want"])
    group = opt.state_dict()["param_groups"][0]
    assert group["avg_steps"] == 3 and group["ema_decay"] == DECAY
    assert not _same(got, _params(m))


def test_surface_swap_in_and_out_and_the_step_after():
    trained = _trained(twins=2)
    m, opt, m2, opt2, batch = (trained[k] for k in ("m", "opt", "m2", "opt2", "batch"))
    p_before, a_before = _params(m), _avg(m, opt)
    assert _same(p_before, _params(m2)) and _same(a_before, _avg(m2, opt2)), "the twins took the same steps"
    with opt.averaged_weights():
        inside = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items() if k in a_before}
        assert _same(inside, a_before)
        with pytest.raises(L.AewError):
            opt.step()
        with pytest.raises(L.AewError):
            with opt.averaged_weights():
                pass
        assert m._engine.averaged_in
    assert not m._engine.averaged_in
    assert _same(_params(m), p_before) and _same(_avg(m, opt), a_before)
    try:                                                            # an exception inside still swaps back
        with opt.averaged_weights():
            raise KeyError("x")
    except KeyError:
        pass
    assert _same(_params(m), p_before) and _same(_avg(m, opt), a_before)
    _step(m, opt, batch)
    _step(m2, opt2, batch)
    assert not _same(_params(m), p_before)
    assert _same(_params(m), _params(m2)) and _same(_avg(m, opt), _avg(m2, opt2))


def test_forward_and_sampler_see_the_averaged_weights(trained):
    from ae_wavenet_amd import mfcc_inverter as mi
    m, opt, batch, hps = (trained[k] for k in ("m", "opt", "batch", "hps"))
    one = [t[:1] for t in batch]
    avg = _avg(m, opt)
    raw_logits = m(*batch).clone()
    raw_wav = m.sample(*one, seed=7).clone()
    with opt.averaged_weights():
        logits = m(*batch).clone()
        wav = m.sample(*one, seed=7).clone()                        # (the B = 1 engine: the swapped state travels with it)
        fresh = mi.MfccInverter(hps).to(DEV)
        fresh.load_state_dict(m.state_dict())
    assert _same({k: v for k, v in _params(fresh).items()}, avg)
    assert bits(fresh(*batch)) == bits(logits)
    assert bits(fresh.sample(*one, seed=7)) == bits(wav)
    assert bits(logits) != bits(raw_logits) and bits(wav) != bits(raw_wav)
    # and out of the context the raw weights compute again
    assert bits(m(*batch)) == bits(raw_logits)
    assert bits(m.sample(*one, seed=7)) == bits(raw_wav)


def test_average_survives_engine_rebuilds(trained):
    m, opt, batch = (trained[k] for k in ("m", "opt", "batch"))
    m(*batch)
    p_ref, a_ref = _params(m), _avg(m, opt)
    steps = opt.state_dict()["param_groups"][0]["avg_steps"]

    def same():
        return _same(_avg(m, opt), a_ref) and _same(_params(m), p_ref) and \
            opt.state_dict()["param_groups"][0]["avg_steps"] == steps
    m.override(n_win_batch=64)                                      # no engine: the model carries the average
    assert m._engine is None and same()
    m.override(n_win_batch=96)
    m(*batch)
    assert m._engine is not None and same()
    m._ensure_engine(3)                                             # another batch size, and back
    assert same()
    m(*batch)
    assert m._engine.B == 2 and same()
    m.to("cpu")
    assert same()
    m.to(DEV)
    with opt.averaged_weights():                                    # no engine live: the sampling engine takes the carry in
        assert m._engine is not None and m._engine.B == 1 and _same(_params(m), a_ref)
        m(*batch)                                                   # another batch size inside: the swapped state travels
        assert m._engine.B == 2 and _same(_params(m), a_ref)
        for gone in (lambda: m.override(n_win_batch=64), lambda: m.to("cpu")):
            with pytest.raises(L.AewError):                         # the engine may change inside, it may not go away
                gone()
        assert m._engine is not None and m._engine.averaged_in
    assert same()
    _step(m, opt, batch)
    assert opt.state_dict()["param_groups"][0]["avg_steps"] == steps + 1 and not _same(_avg(m, opt), a_ref)
