"""Parameter groups on the GPU, through ctypes -> C ABI: the grouped Adam launch (AEW_OP_ADAM_GROUPS) bit for bit against
the plain launch run tensor by tensor, split launches, a uniform table against no table, poisoned frozen tensors, the
argument checks; then the engine / FusedAdam surface on a small model and both data-parallel schedules over RCCL."""
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
from tests.test_update_ratio_cpu import padded_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = L.UW_CHUNK
# shorter than a float4, pad elements, an exact chunk, a chunk plus one, several chunks with a ragged end, and a buffer end
# that is no multiple of 4
SIZES = [1, 3, 4, 5, 1023, 4096, 4097, 8195]
OFFS, TOTAL = padded_offsets(SIZES)
N = OFFS[-1] + SIZES[-1]
P = len(SIZES)
assert N % 4 == 3 and CH == 4096
CANARY = -12345.5
LRS = (1e-3, 3e-4)
# alternating frozen, two rates, decay on some tensors: (lr, weight_decay, frozen)
RECORDS = [(LRS[t % 3 == 0], 0.1 if t in (0, 3, 4, 6) else 0.0, t % 2 == 1) for t in range(P)]
TRAINABLE = [(LRS[t % 2], 0.1 if t in (0, 3, 5, 6, 7) else 0.0, False) for t in range(P)]
UNIFORM = [(1e-3, 0.0, False)] * P


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def pad_end(t):
    return min(OFFS[t] + (SIZES[t] + 3) // 4 * 4, N)


class GFlat:
    """A synthetic flat buffer (SIZES at padded offsets; random p / g / m / v / avg, pads included) between canaries, its
    chunk table, a device table of tensor records and the tracked launch's sums."""

    def __init__(self, seed=0, records=RECORDS, clip=None):
        self.lib = L.load()
        gen = torch.Generator().manual_seed(seed)
        self.state0 = [torch.randn(N, generator=gen), torch.randn(N, generator=gen) * 0.1,
                       torch.randn(N, generator=gen) * 0.01, torch.rand(N, generator=gen) * 1e-3, torch.randn(N, generator=gen)]
        self.bufs = [torch.full((N + 9,), CANARY, device=DEV) for _ in range(5)]     # 4 canaries in front, 5 behind: N + 4 + 5
        self.p, self.g, self.m, self.v, self.avg = (b[4:4 + N] for b in self.bufs)
        self.reset()
        self.chunks_host, self.first_host = L.uw_chunks(OFFS, SIZES)
        self.nch = self.first_host[-1]
        self.chunks = torch.frombuffer(bytearray(bytes(self.chunks_host))[:16 * self.nch], dtype=torch.int64).to(DEV)
        self.part = torch.full((2 * self.nch,), float("nan"), dtype=torch.float64, device=DEV)
        self.clip = None if clip is None else torch.tensor(clip, dtype=torch.float32, device=DEV)
        self.tbl = torch.zeros(4 * P, dtype=torch.int32, device=DEV)
        self.set_records(records)
        gr = self.gr = L.AdamGroups()
        gr.chunks, gr.chunks_host, gr.n_chunks = self.chunks.data_ptr(), C.addressof(self.chunks_host), self.nch
        gr.tensors, gr.n_tensors = self.tbl.data_ptr(), P
        tr = self.tr = L.UwTrack()
        tr.chunks, tr.chunks_host, tr.n_chunks, tr.part = gr.chunks, gr.chunks_host, self.nch, self.part.data_ptr()

    def set_records(self, records):
        self.records = records
        raw = L.adam_tensor_records(records, P)
        self.tbl.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int32))
        self.decay = np.frombuffer(raw, np.float32).reshape(P, 4)[:, 1].copy()

    def reset(self):
        for b, t, s in zip(self.bufs, (self.p, self.g, self.m, self.v, self.avg), self.state0):
            b.fill_(CANARY)
            t.copy_(s)

    def canaries_intact(self):
        return all((b[:4] == CANARY).all().item() and (b[4 + N:] == CANARY).all().item() for b in self.bufs)

    def rec(self, lo=0, hi=N, groups=True, track=False, zero=True, lr=1e-3, t=1, rate=None):
        a = L.Adam()
        a.p, a.g, a.m, a.v = (x.data_ptr() + 4 * lo for x in (self.p, self.g, self.m, self.v))
        a.n = hi - lo
        a.lr, a.beta1, a.beta2, a.eps, a.grad_scale = lr, 0.9, 0.999, 1e-8, 0.5
        a.bc1, a.bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
        a.clip = None if self.clip is None else self.clip.data_ptr()
        if rate is not None:
            a.avg, a.avg_rate = self.avg.data_ptr() + 4 * lo, rate
        if track:
            self.tr.base, self.tr.zero = lo, int(zero)
            a.track = C.addressof(self.tr)
        if not groups:
            return a
        self.gr.base = lo
        ag = L.AdamGrouped()
        ag.adam, ag.groups = a, C.addressof(self.gr)
        return ag

    def adam(self, **kw):
        rec = self.rec(**kw)
        pl = Plan("adam")
        pl.add(L.OP_ADAM_GROUPS if isinstance(rec, L.AdamGrouped) else L.OP_ADAM, rec, "adam")
        pl.run(stream())
        torch.cuda.synchronize()

    def rc(self, rec):
        op = L.Op()
        op.kind = L.OP_ADAM_GROUPS
        op.u.adamg = rec
        fail = C.c_int(-1)
        rc = self.lib.aew_run_plan(C.byref(op), 1, C.c_void_p(stream()), C.byref(fail))
        torch.cuda.synchronize()
        return rc

    def state(self):
        return [bits(b) for b in self.bufs]

    def parents_step(self, t=1, rate=None):
        """The yardstick: the PLAIN launch (no record: the kernel that has always run), tensor by tensor as range calls
        with that tensor's lr, on parameters that torch multiplied by decay_t on the device (one fp32 multiply); frozen
        tensors are left out."""
        for k, (lr, wd, frozen) in enumerate(self.records):
            if frozen:
                continue
            lo, hi = OFFS[k], pad_end(k)
            if self.decay[k] != np.float32(1.0):
                torch.mul(self.p[lo:hi], torch.tensor(self.decay[k], device=DEV), out=self.p[lo:hi])
            self.adam(lo=lo, hi=hi, groups=False, lr=lr, t=t, rate=rate)


# ----------------------------------------------------------------------------------------------
# op level
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", [RECORDS, TRAINABLE], ids=["alternating frozen", "last tensor trainable"])
@pytest.mark.parametrize("clip,rate,track", [(None, None, False), ([0.37, 0.0], 0.25, False), (None, 0.25, True), ([0.37, 0.0], None, True)])
def test_grouped_launch_against_the_plain_launch_tensor_by_tensor(records, clip, rate, track):
    a, b = GFlat(3, records, clip=clip), GFlat(3, records, clip=clip)
    assert a.decay[0] == np.float32(1.0 - records[0][0] * 0.1) != 1.0 and len({r[0] for r in records}) == 2
    for t in (1, 2):
        old = a.p.clone()
        a.adam(t=t, rate=rate, track=track)
        b.parents_step(t=t, rate=rate)
        assert a.state() == b.state(), (t, [k for k in range(5) if bits(a.bufs[k]) != bits(b.bufs[k])])
        if track:                                                   # frozen: 0 / the true weight norm; p_old in front of the decay
            part = a.part.cpu().numpy().reshape(-1, 2)
            o, n = old.cpu().numpy(), a.p.cpu().numpy()
            for k in range(P):
                c0, c1 = a.first_host[k], a.first_host[k + 1]
                d = (o[OFFS[k]:OFFS[k] + SIZES[k]] - n[OFFS[k]:OFFS[k] + SIZES[k]]).astype(np.float64)
                w = o[OFFS[k]:OFFS[k] + SIZES[k]].astype(np.float64)
                assert abs(part[c0:c1, 1].sum() / (w * w).sum() - 1) < 1e-11, k
                if records[k][2]:
                    assert (part[c0:c1, 0] == 0.0).all(), k
                else:
                    assert abs(part[c0:c1, 0].sum() / (d * d).sum() - 1) < 1e-11 and (d * d).sum() > 0, k
    assert a.canaries_intact()
    s0 = a.state0
    for k in range(P):
        lo, hi = OFFS[k], pad_end(k)
        same = [bits(x[lo:hi]) == s[lo:hi].numpy().tobytes() for x, s in zip((a.p, a.m, a.v, a.avg), (s0[0], s0[2], s0[3], s0[4]))]
        assert same == ([True] * 4 if records[k][2] else [False, False, False, rate is None]), (k, same)


# 4100 and 4096 lie inside the one chunk of the tensor of 4096 elements (flat offsets 1044 .. 5140); 5140 is a tensor
# boundary, 9236 the edge in front of a chunk of one element, 13336 a chunk edge inside the last tensor
@pytest.mark.parametrize("cut", [4100, 4096, 5140, 9236, 13336])
@pytest.mark.parametrize("track", [False, True])
def test_split_launch_against_the_whole_launch(cut, track):
    """The same step as two range calls, cut inside a chunk and on chunk edges."""
    edges = [OFFS[k] + c * CH for k in range(P) for c in range((SIZES[k] + CH - 1) // CH)]
    assert cut % 4 == 0 and (cut in edges) == (cut in (5140, 9236, 13336))
    f = GFlat(5, TRAINABLE)
    f.adam(rate=0.25, track=track)
    whole, part = f.state(), bits(f.part)
    f.reset()
    f.adam(lo=cut, hi=N, rate=0.25, track=track, zero=True)          # the order of a data-parallel step: tail first
    f.adam(lo=0, hi=cut, rate=0.25, track=track, zero=False)
    assert f.state() == whole and f.canaries_intact()
    if track:
        got, want = np.frombuffer(bits(f.part), np.float64), np.frombuffer(part, np.float64)
        assert np.abs(got / want - 1).max() < 1e-12                  # (a cut chunk adds its two halves: another fp64 order)
    # one range alone leaves everything outside it alone
    f.reset()
    before = [b.cpu().numpy().copy() for b in f.bufs]
    f.adam(lo=cut, hi=cut + 8, rate=0.25)
    for k, (b, w) in enumerate(zip(f.bufs, whole)):
        got, want = b.cpu().numpy(), np.frombuffer(w, np.float32)
        sl = slice(4 + cut, 12 + cut)
        assert got[sl].tobytes() == want[sl].tobytes(), k
        got[sl] = before[k][sl]
        assert got.tobytes() == before[k].tobytes(), k


@pytest.mark.parametrize("clip,rate,track", [(None, None, False), ([0.5, 0.0], 0.25, True)])
def test_null_groups_against_a_uniform_table(clip, rate, track):
    a, b = GFlat(7, UNIFORM, clip=clip), GFlat(7, UNIFORM, clip=clip)
    assert (a.decay == np.float32(1.0)).all()
    for t in (1, 2):
        a.adam(groups=False, t=t, rate=rate, track=track)
        b.adam(groups=True, lr=123.0, t=t, rate=rate, track=track)   # (with a table the descriptor's lr is not read)
        assert a.state() == b.state(), t
        if track:
            assert bits(a.part) == bits(b.part), t
    assert not torch.equal(a.p.cpu(), a.state0[0])


@pytest.mark.parametrize("track", [False, True])
def test_poisoned_frozen_tensors_keep_their_nans_to_themselves(track):
    f = GFlat(9, RECORDS)
    poison = torch.zeros(N, dtype=torch.bool)
    for k in range(P):
        if RECORDS[k][2]:
            poison[OFFS[k]:pad_end(k)] = True
    for x in (f.g, f.m, f.v, f.avg):
        x[poison.to(DEV)] = float("nan")
    clean = GFlat(9, RECORDS)
    f.adam(rate=0.25, track=track)
    clean.adam(rate=0.25, track=track)
    for x, y in zip((f.g, f.m, f.v, f.avg), (clean.g, clean.m, clean.v, clean.avg)):
        got = x.cpu()
        assert torch.isnan(got[poison]).all() and not torch.isnan(got[~poison]).any()
        assert bits(got[~poison]) == bits(y.cpu()[~poison])
    assert bits(f.p) == bits(clean.p) and not torch.isnan(f.p).any() and f.canaries_intact()
    if track:
        assert bits(f.part) == bits(clean.part) and not torch.isnan(f.part).any()
    # a skipped step (the clip flag) leaves a grouped launch's buffers alone as well
    s = GFlat(9, TRAINABLE, clip=[0.5, 1.0])
    old = s.state()
    s.adam(rate=0.25, track=track)
    assert s.state() == old


def test_refused_descriptors_write_nothing():
    f = GFlat(11, TRAINABLE)
    old = f.state()
    a = f.rec(lo=4)
    f.gr.base = 6                                                   # base % 4
    assert f.rc(a) == L.E_ALIGN
    a = f.rec()
    f.gr.base = -4
    assert f.rc(a) == L.E_ARG
    for field in ("chunks", "chunks_host", "tensors"):               # NULL tables
        a = f.rec()
        keep = getattr(f.gr, field)
        setattr(f.gr, field, None)
        assert f.rc(a) == L.E_ARG, field
        setattr(f.gr, field, keep)
    a = f.rec()
    f.gr.tensors = f.tbl.data_ptr() + 4
    assert f.rc(a) == L.E_ALIGN
    f.gr.tensors = f.tbl.data_ptr()
    a = f.rec()
    f.gr.n_chunks = f.nch - 1                                       # the chunks do not cover [base, base + n)
    assert f.rc(a) == L.E_ARG
    f.gr.n_chunks = f.nch
    a = f.rec()
    a.adam.n = N + 4
    assert f.rc(a) == L.E_ARG
    a = f.rec()
    a.groups = None                                                 # no record at all
    assert f.rc(a) == L.E_ARG
    a = f.rec()
    a.adam.p = f.p.data_ptr() + 4                                    # what AEW_OP_ADAM refuses
    assert f.rc(a) == L.E_ALIGN
    a = f.rec()
    f.gr.n_tensors = P - 1                                          # a chunk names a tensor outside the table
    assert f.rc(a) == L.E_ARG
    f.gr.n_tensors = P
    a = f.rec(track=True)
    f.tr.base = 4                                                   # track and groups disagree
    assert f.rc(a) == L.E_ARG
    assert f.state() == old and torch.isnan(f.part).all()           # every refusal comes before any launch
    assert f.rc(f.rec(track=True)) == 0 and f.state() != old
    lib = L.load()
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(11) == C.sizeof(L.Adam)
    assert lib.aew_sizeof(29) == C.sizeof(L.AdamTensor) == 16 and lib.aew_sizeof(30) == C.sizeof(L.AdamGroups)
    assert lib.aew_sizeof(31) == C.sizeof(L.AdamGrouped)


# ----------------------------------------------------------------------------------------------
# model level: the tiny configuration of the optimizer GPU tests (tests/test_weight_avg_gpu.py)
# ----------------------------------------------------------------------------------------------
GROUPS = [dict(params=["encoder.*", "bottleneck.*"], frozen=True),
          dict(params="decoder.*.bias", lr=5e-4),
          dict(params="decoder.*", lr=2e-4, weight_decay=0.1)]


def _ae(seed=3):
    from ae_wavenet_amd import autoencoder_model as ae, config
    hps = config.make_hps("vqvae-ema", n_res=64, n_dil=32, n_skp=32, n_post=32, n_lc_out=16, enc_n_out=64, bn_n_out=8,
                          bn_vq_n_embed=64, n_win_batch=96, n_blocks=2, n_block_layers=3, n_global_embed=4, n_speakers=5)
    torch.manual_seed(seed)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    g = m.geom
    gen = torch.Generator().manual_seed(2)
    batch = (torch.randint(0, 256, (2, g.enc_in_len), generator=gen).float().to(DEV),
             torch.randn(2, 39, g.mel_len, generator=gen).to(DEV),
             torch.randint(0, 5, (2,), generator=gen).to(DEV), torch.arange(g.embed_len).repeat(2, 1).to(DEV))
    return m, batch


def _frozen_name(k):
    return k.startswith(("encoder.", "bottleneck."))


def test_model_three_steps_frozen_bits_the_plain_launch_replay_and_the_trainable_norm():
    """3 steps of run / backward / step with the three-group optimizer, clipping, tracking and the average.  After every
    step: the grouped step equals, bit for bit, a replay on a twin engine of the emulator's rule (tests/
    adam_groups_emulator.py: tensor by tensor, p * decay_t as one fp32 multiply, then the step WITHOUT a record with lr_t) run
    with the plain device launch on the same gradients and the same clip word - the element update itself (rsqrtf, the
    division) has no bit-exact host restatement, so the device's own plain launch stands in for it, as at op level;
    opt.grad_norm is the norm of the trainable gradients computed by torch on the device (relative 1e-6: the op sums in
    fp64, torch's fp32 norm is the looser side)."""
    from ae_wavenet_amd import model as M, optim
    m, batch = _ae()
    opt = optim.FusedAdam(m, lr=1e-3, max_grad_norm=0.05, track_update_ratio=True, ema_decay=0.9, groups=GROUPS)
    eng = m._ensure_engine(2)
    twin = M.TrainEngine(m.hps, 2, m._device, n_win=m.window_batch_size, **m._opts)
    n = eng.ps.numel
    names = eng.ps.names()
    assert names == [k for k, _ in m.named_parameters()]
    twin.ps.params[:n].copy_(eng.ps.params[:n])
    start = eng.ps.params[:n].clone()
    for step in range(3):
        opt.param_groups[2]["lr"] = 2e-4 / (1 + step)                 # a per-group schedule
        opt.zero_grad()
        m.run(*batch)[2].backward()
        grads = eng.ps.grads[:n].clone()
        rec = opt._tensor_records()
        opt.step()
        trainable = [p.grad for k, p in m.named_parameters() if not _frozen_name(k)]
        want = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in trainable])))
        assert abs(float(opt.grad_norm) / want - 1) < 1e-6, (step, float(opt.grad_norm), want)
        assert 0.0 < float(opt.clip_coef) < 1.0
        # the replay: the clip word of the grouped step, the plain launch per trainable tensor
        twin.ps.grads[:n].copy_(grads)
        twin.clip_out[:4].copy_(eng.clip_out[:4])
        decay = np.frombuffer(L.adam_tensor_records(rec, len(rec)), np.float32).reshape(-1, 4)[:, 1]
        first = True
        rate = optim.ema_rate_at(0.9, step)
        for k, (lo, hi), r in zip(names, eng._tensor_span, rec):
            if r[2]:
                continue
            if first and step == 0:                                 # the average starts from the parameters in front of step 1
                twin._avg_buffer()[:n].copy_(start)
                twin.avg_live = True
            if decay[names.index(k)] != np.float32(1.0):
                torch.mul(twin.ps.params[lo:hi], torch.tensor(decay[names.index(k)], device=DEV), out=twin.ps.params[lo:hi])
            twin.adam_step(r[0], 1.0, lo=lo, hi=hi, count=first, max_grad_norm=0.05, norm_done=True, avg_rate=rate)
            first = False
        torch.cuda.synchronize()
        for what, a, b in (("p", eng.ps.params, twin.ps.params), ("m", eng.adam_m, twin.adam_m), ("v", eng.adam_v, twin.adam_v),
                           ("avg", eng.adam_avg, twin.adam_avg)):
            assert bits(a[:n]) == bits(b[:n]), (step, what)
    un, wn, ur = opt.update_norm, opt.weight_norm, opt.update_ratio
    moved = 0
    for k, (lo, hi) in zip(names, eng._tensor_span):
        same = [bits(x[lo:hi]) == bits(y[lo:hi]) for x, y in ((eng.ps.params, start), (eng.adam_avg, start))]
        if _frozen_name(k):
            assert same == [True, True] and not eng.adam_m[lo:hi].any() and not eng.adam_v[lo:hi].any(), k
            w = float(start[lo:lo + eng.ps.numel_of(k)].double().norm())
            assert float(un[k]) == 0.0, k
            if w > 0:
                assert float(ur[k]) == 0.0 and abs(float(wn[k]) / w - 1) < 1e-6, k
            else:                                                   # a zero-initialised bias: 0 / 0, the plain fp32 division
                assert float(wn[k]) == 0.0 and np.isnan(float(ur[k])), k
        else:
            assert same == [False, False] and float(un[k]) > 0.0, k
            moved += 1
    assert moved > 10 and len(names) - moved > 10


def test_freezing_all_but_one_tensor_makes_the_norm_that_tensors_alone():
    from ae_wavenet_amd import optim
    m, batch = _ae()
    opt = optim.FusedAdam(m, lr=1e-3, max_grad_norm=1e-3, groups=[dict(params="decoder.post1.weight"), dict(params="*", frozen=True)])
    p = dict(m.named_parameters())["decoder.post1.weight"]
    opt.zero_grad()
    m.run(*batch)[2].backward()
    opt.step()
    want, total = float(torch.linalg.vector_norm(p.grad)), float(torch.linalg.vector_norm(m._engine.ps.grads[:m._engine.ps.numel]))
    assert abs(float(opt.grad_norm) / want - 1) < 1e-6 and want < 0.9 * total
    # requires_grad_(False) on the only trainable tensor: nothing is left, the norm is 0 and nothing moves
    before = bits(m._engine.ps.params[:m._engine.ps.numel])
    p.requires_grad_(False)
    opt.zero_grad()
    m.run(*batch)[2].backward()
    opt.step()
    assert float(opt.grad_norm) == 0.0 and bits(m._engine.ps.params[:m._engine.ps.numel]) == before


def test_five_steps_against_torch_adamw_on_device_tensors():
    """The worst relative distance of the grouped step from torch.optim.AdamW with the same groups may be at most twice
    the distance the ungrouped FusedAdam shows from torch.optim.Adam on the same gradients (one extra rounding per step;
    the kernel's rsqrtf and division are the same in both).  Both are printed, and appended to the file AEW_GROUPS_REPORT
    names where it is set (profiles/adam_groups.txt holds a run's line)."""
    from ae_wavenet_amd import optim
    dist = {}
    for how in ("plain", "grouped"):
        m, batch = _ae()
        if how == "plain":
            opt = optim.FusedAdam(m, lr=1e-3)
            ref = {k: torch.nn.Parameter(p.detach().clone()) for k, p in m.named_parameters()}
            stock = torch.optim.Adam(list(ref.values()), lr=1e-3)
        else:
            opt = optim.FusedAdam(m, lr=1e-3, groups=GROUPS)
            ref = {k: torch.nn.Parameter(p.detach().clone()) for k, p in m.named_parameters()}
            idx = {id(p): k for k, p in m.named_parameters()}
            stock = torch.optim.AdamW([dict(params=[ref[idx[id(p)]] for p in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"])
                                       for g in opt.param_groups if not g["frozen"]], lr=1e-3)
        for step in range(5):
            opt.zero_grad()
            m.run(*batch)[2].backward()
            for k, p in m.named_parameters():
                ref[k].grad = p.grad.detach().clone()
            opt.step()
            stock.step()
        worst = 0.0
        for k, p in m.named_parameters():
            if how == "grouped" and _frozen_name(k):
                assert torch.equal(p.detach(), ref[k].detach()), k
                continue
            d = float((p.detach() - ref[k].detach()).abs().max() / ref[k].detach().abs().max())
            worst = max(worst, d)
        dist[how] = worst
    line = f"distance from torch after 5 steps, max |p - p_torch| / max |p_torch| per tensor: plain FusedAdam vs Adam " \
           f"{dist['plain']:.3e}, grouped vs AdamW {dist['grouped']:.3e}"
    print(line)
    report = os.environ.get("AEW_GROUPS_REPORT")
    if report:
        with open(report, "a") as f:
            f.write(line + "\n")
    assert dist["grouped"] <= 2 * dist["plain"], line


@pytest.mark.parametrize("schedule", ["allreduce", "sharded"])
def test_schedules_over_rccl_on_one_rank(schedule):
    """RCCL ("nccl"), one rank, DataParallel(force_collectives=True): the schedule's own step with the group record
    against the unsharded engine.  tests/adam_groups_rccl_one_rank.py runs it in a fresh process."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "adam_groups_rccl_one_rank.py"), schedule], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    out = json.loads(lines[-1])
    assert out["backend"] == "nccl" and out["world"] == 1 and out["schedule"] == schedule
    # (sharded: one call per exchanged region - decoder and head at least - even on one rank; all-reduce: the whole buffer)
    assert out["adam_calls"] >= (2 if schedule == "sharded" else 1) * out["steps"]
    assert out["frozen_tensors"] > 10 and out["frozen_still"] and out["moved"], out
    assert out["norm_rel"] < 1e-6 and out["coefs"] == [1.0] * out["steps"], out
    assert out["bit_equal"] == {"params": True, "m": True, "v": True}, out
