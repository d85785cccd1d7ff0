"""TEST INFRASTRUCTURE - one-op plans of the step's non-GEMM ops: buffers, descriptors, expectations.

Shared by tests/test_step_ops_cpu.py (the plan interpreter) and tests/test_step_ops_gpu.py (the HIP kernels), so that
both see literally the same bytes.  A case builds a CPU Workspace whose buffers are filled end to end with non-zero
canary values and then with the inputs; `ops(ws)` makes the descriptors against a workspace (the CPU one or its device
mirror); `expect()` lists, from tests/step_ops_reference.py alone, every element the op must write - its fp64 value and
the sum S of the absolute values of the terms it adds up.  `verify` holds the written elements to their rule and every
other byte of every buffer (guards, pads, inputs, rows no op should touch) to bit identity with the state before.

Rules (S: the sum of the absolute values of the terms an element adds up, from the fp64 reference):
  exact      S is None: bit for bit
  fp32 sum   |got - ref| <= (n + c) 2^-24 S         n terms, c = 16 operations around them (2d + 16 through two norms)
  bf16 out   ... + 2^-7 |ref|                       one bf16 spacing
  intrinsic  outputs behind __expf / __logf: on the GPU the coefficient of S is a measured constant (test_step_ops_gpu),
             on the CPU (fp32 torch, no fast intrinsics) the derived (n + c) 2^-24 with the n given here
  every computed output may also be off by 2^-126: values below the smallest normal float may be flushed to zero
"""
import numpy as np
import torch

from ae_wavenet_amd import _lib as L
from ae_wavenet_amd.plan import Workspace
from tests import step_ops_reference as R

GUARD = 64
U = 2.0 ** -24
TINY = 2.0 ** -126
NP2T = {np.float32: torch.float32, np.int64: torch.int64, np.int32: torch.int32}


class Expect:
    def __init__(self, buf, idx, ref, S=None, n=0, c=16, tag="", extra=0.0):
        self.buf, self.n, self.c, self.tag, self.extra = buf, n, c, tag, extra
        self.idx, self.ref = np.asarray(idx).reshape(-1), np.asarray(ref).reshape(-1)
        self.S = None if S is None else np.broadcast_to(np.asarray(S, dtype=np.float64), np.shape(ref)).reshape(-1)
        assert self.idx.shape == self.ref.shape, (buf, tag, self.idx.shape, self.ref.shape)


class Case:
    """Subclasses: fill(self) -> allocate with self.buf(), ops(self, ws) -> [(kind, payload, label)], expect(self) -> [Expect]"""
    seed = 1

    def build(self):
        self.ws = Workspace("cpu")
        self.rng = np.random.default_rng(self.seed)
        self.len = {}
        self.fill()
        return self.ws

    def buf(self, name, data, dtype=None, n=None):
        """A buffer of GUARD canaries | payload | GUARD canaries (+ the workspace's own slack), payload = data."""
        if data is not None:
            data = np.ascontiguousarray(data).reshape(-1)
            n = data.size
        tdt = dtype if dtype is not None else NP2T[data.dtype.type]
        t = self.ws.alloc(name, GUARD + n + GUARD, tdt, zero=False)
        t.copy_(self.canary(t.numel(), tdt))
        if data is not None:
            t[GUARD:GUARD + n] = torch.from_numpy(data).to(tdt)
        self.len[name] = n
        return t

    def canary(self, n, tdt):
        if tdt in (torch.int64, torch.int32):
            return torch.full((n,), -77, dtype=tdt)
        v = self.rng.uniform(1.0, 2.0, n) * self.rng.choice([-1.0, 1.0], n)
        return torch.from_numpy(v).to(tdt)

    def uni(self, shape, lo=-1.0, hi=1.0):
        return self.rng.uniform(lo, hi, shape).astype(np.float32)


def P(ws, name, off=0):
    return ws.ptr(name, GUARD + off)


def snapshot(ws):
    return {n: t.detach().cpu().clone() for n, t in ws.bufs.items()}


def clone_ws(ws, device="cpu"):
    out = Workspace(device)
    for n, t in ws.bufs.items():
        out.bufs[n] = t.clone() if device == "cpu" else t.to(device)
    return out


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def verify(case, before, after, coef=None, report=None, what=""):
    """coef: {tag: coefficient of S} overriding the derived (n + c) 2^-24 (the measured GPU constants); report: dict that
    receives the worst (err - extra) / S per tag.  Returns nothing; raises AssertionError with the first offender."""
    touched = {n: np.zeros(t.numel(), dtype=bool) for n, t in before.items()}
    for e in case.expect():
        at = GUARD + e.idx
        assert not touched[e.buf][at].any(), ("element expected twice", e.buf, e.tag)
        touched[e.buf][at] = True
        got_t = after[e.buf][torch.from_numpy(at)]
        if e.S is None:
            want_t = torch.from_numpy(e.ref).to(got_t.dtype)
            assert (want_t.double().numpy() == e.ref.astype(np.float64)).all(), ("reference not representable", e.buf, e.tag)
            bad = (_bits(got_t) != _bits(want_t)).nonzero()
            assert bad.numel() == 0, (what, case.name, e.buf, e.tag, "exact rule: first mismatch at element", int(e.idx[int(bad[0])]),
                                      "got", float(got_t[int(bad[0])]), "want", float(want_t[int(bad[0])]), "mismatches", int(bad.shape[0]))
            continue
        got = got_t.double().numpy()
        assert np.isfinite(got).all(), (what, case.name, e.buf, e.tag, "non-finite output")
        err = np.abs(got - e.ref)
        extra = np.asarray(e.extra, dtype=np.float64) + TINY
        k = coef[e.tag] if coef and e.tag in coef else (e.n + e.c) * U
        if report is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(e.S > 0, np.clip(err - extra, 0, None) / e.S, 0.0)
            report[e.tag] = max(report.get(e.tag, 0.0), float(r.max()) if r.size else 0.0)
        over = err > k * e.S + extra
        if over.any():
            i = int(np.argmax(err - (k * e.S + extra)))
            raise AssertionError((what, case.name, e.buf, e.tag, "element", int(e.idx[i]), "got", got[i], "ref", e.ref[i], "err", err[i],
                                  "bound", float(k * e.S[i] + np.broadcast_to(extra, err.shape)[i]), "over", int(over.sum())))
    for n, t in before.items():
        keep = torch.from_numpy(~touched[n])
        bad = (_bits(t)[keep] != _bits(after[n])[keep]).nonzero()
        assert bad.numel() == 0, (what, case.name, n, "an element no op should touch changed: index (with guard)",
                                  int(keep.nonzero()[int(bad[0])]), "changed", int(bad.shape[0]))


def grid(*dims):
    """flat offsets of a strided box: grid((n0, s0), (n1, s1), ...) -> array of shape (n0, n1, ...)"""
    out = np.zeros((), dtype=np.int64)
    for n, s in dims:
        out = out[..., None] + np.arange(n, dtype=np.int64) * s
    return out


# =================================================================================================
class SoftmaxCase(Case):
    B, w, tgt_off = 3, 9, 2

    def __init__(self, Q, Q_pad, pitch, backward, gmul=None, peak=False):
        self.Q, self.Q_pad, self.pitch, self.backward, self.gmul, self.peak = Q, Q_pad, pitch, backward, gmul, peak
        self.name = f"softmax Q{Q} pad{Q_pad} pitch{pitch} {'bwd' if backward else 'fwd'} gmul={gmul} peak={peak}"
        self.seed = 100 + Q                                   # the same data for every pitch / direction of a class count
        self.bs = self.w * pitch + 8
        self.wav_pitch = self.w + 7
        self.dl_pitch = Q_pad + 8
        self.dl_bs = self.w * self.dl_pitch + 8
        self.scale = float(np.float32(1.0 / (self.B * (self.w - 1))))

    def register_path(self):
        return self.Q == 256 and self.Q_pad == 256 and self.pitch % 4 == 0 and self.bs % 4 == 0

    def fill(self):
        B, w, Q = self.B, self.w, self.Q
        lg = self.uni((B, w, Q), -4, 4)
        lg[0, 1] = self.rng.permutation(np.linspace(-80, 80, Q)).astype(np.float32)   # one row spread over +-80
        lg[0, 2] = 1.5                                                             # all equal
        lg[1, 0, 8] = lg[1, 0, 10] = 9.0       # the maximum twice in one lane's group of four (classes 8..11)
        lg[1, 1, 5] = lg[1, 1, Q - 3] = 9.0    # the maximum in two lanes: the lowest class wins
        lg[2, 3, 0] = 7.0                      # maximum at class 0 and at class Q - 1
        lg[2, 4, Q - 1] = 7.0
        self.lg = lg
        wav = self.rng.integers(0, Q, (B, self.wav_pitch))
        wav[0, self.tgt_off + 1], wav[0, self.tgt_off + 2], wav[1, self.tgt_off + 1] = 0, Q - 1, 8
        wav[1, self.tgt_off + 2] = Q - 3
        self.wav = wav
        full = np.full((B, self.bs), 50.0, dtype=np.float32)                        # pad columns: large, must not be read
        full.reshape(-1)[grid((B, self.bs), (w, self.pitch), (Q, 1))] = lg
        self.buf("logits", full)
        self.buf("wav", wav.astype(np.float32))
        for n in ("nll", "ptgt", "peak"):
            self.buf(n, None, torch.float32, B * w)
        self.buf("amax", None, torch.int32, B * w)
        self.buf("dlogits", None, torch.bfloat16, B * self.dl_bs)
        self.buf("gmul", np.array([self.gmul or 0.0] * 4, dtype=np.float32))

    def ops(self, ws):
        sm = L.SoftmaxNll()
        sm.logits, sm.bs, sm.pitch = P(ws, "logits"), self.bs, self.pitch
        sm.wav, sm.wav_pitch, sm.tgt_off = P(ws, "wav"), self.wav_pitch, self.tgt_off
        sm.B, sm.w, sm.Q, sm.Q_pad = self.B, self.w, self.Q, self.Q_pad
        sm.nll, sm.ptgt = P(ws, "nll"), P(ws, "ptgt")
        sm.dlogits, sm.dl_bs, sm.dl_pitch = P(ws, "dlogits"), self.dl_bs, self.dl_pitch
        sm.scale, sm.backward = self.scale, int(self.backward)
        if self.gmul is not None:
            sm.gmul = P(ws, "gmul")
        if self.peak:
            sm.peak, sm.amax = P(ws, "peak"), P(ws, "amax")
        return [(L.OP_SOFTMAX_NLL, sm, "softmax")]

    def expect(self):
        B, w, Q = self.B, self.w, self.Q
        lg = self.lg.astype(np.float64)
        mx, se, lsm = R.softmax_parts(lg)
        tgt, live = R._targets(self.wav, self.tgt_off, w)
        # error model: se = sum exp(l - mx) carries (Q + Q / e + few) 2^-24 relative (Q additions, and e^-x x <= 1 / e per term
        # for the rounding of l - mx), log se an absolute error of the same size, mx + log se and l - lse one rounding each:
        # n = 2 Q terms on S = 1 + |l| + |mx| + |log se|
        Sall = 1.0 + np.abs(lg) + (np.abs(mx) + np.abs(np.log(se)))[..., None]
        pos = np.arange(B * w).reshape(B, w)
        if not self.backward:
            nll, ptgt, peak, amax = R.softmax_nll_fwd(lg, self.wav, self.tgt_off)
            St = np.take_along_axis(Sall, tgt[..., None], -1)[..., 0]
            out = [Expect("nll", pos[live], nll[live], St[live], 2 * Q, tag="nll"),
                   Expect("nll", pos[~live], nll[~live]),
                   Expect("ptgt", pos[live], ptgt[live], (ptgt * St)[live], 2 * Q, tag="ptgt"),
                   Expect("ptgt", pos[~live], ptgt[~live])]
            if self.peak:
                out += [Expect("peak", pos, peak, 1.0 + np.abs(mx) + np.abs(np.log(se)), 2 * Q, tag="peak"), Expect("amax", pos, amax)]
            return out
        ref = R.softmax_nll_bwd(lg, self.wav, self.tgt_off, self.scale, self.Q_pad, self.gmul)
        sc = abs(self.scale * (1.0 if self.gmul is None else float(np.float32(self.gmul))))
        S = np.exp(lsm) * Sall
        np.put_along_axis(S, tgt[..., None], np.take_along_axis(S, tgt[..., None], -1) + 1.0, -1)
        idx = grid((B, self.dl_bs), (w, self.dl_pitch), (self.Q_pad, 1))
        lv = np.broadcast_to(live[..., None], (B, w, Q)).copy()
        body = ref[:, :, :Q]
        out = [Expect("dlogits", idx[:, :, :Q][lv], body[lv], (S * sc)[lv], 2 * Q, tag="dlogits", extra=2.0 ** -7 * np.abs(body[lv])),
               Expect("dlogits", idx[:, :, :Q][~lv], body[~lv])]
        if self.Q_pad > Q:
            out.append(Expect("dlogits", idx[:, :, Q:], ref[:, :, Q:]))
        return out


# =================================================================================================
class BaseGatherCase(Case):
    B, wav_off = 2, 3

    def __init__(self, T, R, R_pad, bias, onehot_q, wt):
        self.T, self.R, self.R_pad, self.bias, self.onehot, self.wt = T, R, R_pad, bias, onehot_q is not None, wt
        self.Q = self.Q_pad = onehot_q or 64
        self.name = f"base_gather T{T} R{R}/{R_pad} bias={bias} onehot={onehot_q} Wt={wt}"
        self.seed = 7 + T + R
        self.wav_pitch, self.x_pitch, self.oh_pitch = T + 8, R_pad + 8, self.Q_pad + 8
        self.x_bs, self.oh_bs = T * self.x_pitch + 16, T * self.oh_pitch + 16

    def fill(self):
        B, T, R, Q = self.B, self.T, self.R, self.Q
        self.W = self.uni((R, Q), -2, 2)
        self.bv = self.uni((R,), -1, 1)
        wav = self.rng.integers(0, Q, (B, self.wav_pitch))
        wav[0, self.wav_off], wav[1, self.wav_off] = 0, Q - 1
        self.wav = wav
        Wt = np.zeros((Q, self.R_pad), dtype=np.float32)
        Wt[:, :R] = self.W.T
        self.buf("wav", wav.astype(np.float32))
        self.buf("W", self.W)
        self.buf("Wt", Wt)
        self.buf("bias", self.bv)
        self.buf("x", None, torch.bfloat16, B * self.x_bs)
        self.buf("onehot", None, torch.bfloat16, B * self.oh_bs)

    def ops(self, ws):
        p = L.BaseGather()
        p.wav, p.wav_pitch, p.wav_off = P(ws, "wav"), self.wav_pitch, self.wav_off
        p.W, p.bias, p.Wt = P(ws, "W"), P(ws, "bias") if self.bias else None, P(ws, "Wt") if self.wt else None
        p.B, p.T, p.R, p.R_pad, p.Q, p.Q_pad = self.B, self.T, self.R, self.R_pad, self.Q, self.Q_pad
        p.x, p.x_bs, p.x_pitch = P(ws, "x"), self.x_bs, self.x_pitch
        if self.onehot:
            p.onehot, p.oh_bs, p.oh_pitch = P(ws, "onehot"), self.oh_bs, self.oh_pitch
        p.ones_channel = int(self.R < self.R_pad)
        return [(L.OP_BASE_GATHER, p, "base")]

    def expect(self):
        x, oh = R.base_gather(self.wav, self.wav_off, self.T, self.W, self.bv if self.bias else None, self.R_pad,
                              self.R < self.R_pad, self.Q_pad if self.onehot else None)
        out = [Expect("x", grid((self.B, self.x_bs), (self.T, self.x_pitch), (self.R_pad, 1)), x)]
        if self.onehot:
            out.append(Expect("onehot", grid((self.B, self.oh_bs), (self.T, self.oh_pitch), (self.Q_pad, 1)), oh))
        return out


# =================================================================================================
def jitter_rows(rng, B, N, jit_pitch, shift=0, big=False):
    """row kinds by (b + shift) % 3: identity | all at one row | random with -1, N and N + 3 among the entries.
    big: a permutation with a handful of collisions (the large-N cases)."""
    jit = np.full((B, jit_pitch), 10 ** 6, dtype=np.int64)              # entries behind N: never read
    for b in range(B):
        k = (b + shift) % 3
        if big:
            row = rng.permutation(N)
            row[rng.integers(0, N, 6)] = row[rng.integers(0, N, 6)]
            row[0], row[N - 1] = -1, N + 3
        elif k == 0:
            row = np.arange(N)
        elif k == 1:
            row = np.full(N, N // 2)
        else:
            row = rng.integers(0, N, N)
            for i, v in enumerate((-1, N, N + 3)):
                row[(i * 2) % N] = v
        jit[b, :N] = row
    return jit


class LcGatherCase(Case):
    def __init__(self, B, N, C, C_pad, take, shift=0):
        self.B, self.N, self.C, self.C_pad, self.take, self.shift = B, N, C, C_pad, take, shift
        self.name = f"lc_gather B{B} N{N} C{C}/{C_pad} take={take} shift={shift}"
        self.seed = 11 + B * 100 + N
        self.src_pitch, self.dst_pitch, self.jit_pitch = C + 3, C_pad + 4, N + 5
        self.src_bs, self.dst_bs = N * self.src_pitch + 5, N * self.dst_pitch + 6

    def fill(self):
        B, N, C = self.B, self.N, self.C
        self.src = self.uni((B, N, C), -3, 3)
        self.jit = jitter_rows(self.rng, B, N, self.jit_pitch, self.shift)
        full = self.uni((B, self.src_bs), 5, 6)
        full.reshape(-1)[grid((B, self.src_bs), (N, self.src_pitch), (C, 1))] = self.src
        self.buf("src", full)
        self.buf("jitter", self.jit)
        self.buf("dst", None, torch.bfloat16, B * self.dst_bs)

    def ops(self, ws):
        p = L.LcGather()
        p.src, p.src_bs, p.src_pitch = P(ws, "src"), self.src_bs, self.src_pitch
        p.jitter, p.jit_pitch = P(ws, "jitter"), self.jit_pitch
        p.dst, p.dst_bs, p.dst_pitch = P(ws, "dst"), self.dst_bs, self.dst_pitch
        p.B, p.N, p.C, p.C_pad, p.take_compat = self.B, self.N, self.C, self.C_pad, self.take
        return [(L.OP_LC_GATHER, p, "lc_gather")]

    def expect(self):
        return [Expect("dst", grid((self.B, self.dst_bs), (self.N, self.dst_pitch), (self.C_pad, 1)),
                       R.lc_gather(self.src, self.jit, self.C_pad, self.take))]


class LcScatterCase(Case):
    def __init__(self, B, N, C, take, shift=0, big=False):
        self.B, self.N, self.C, self.take, self.shift, self.big = B, N, C, take, shift, big
        self.name = f"lc_scatter B{B} N{N} C{C} take={take} shift={shift}"
        self.seed = 13 + B * 100 + N
        self.d_pitch, self.dsrc_pitch, self.jit_pitch = C + 2, C + 1, N + 5
        self.d_bs, self.dsrc_bs = N * self.d_pitch + 3, N * self.dsrc_pitch + 7

    def fill(self):
        B, N, C = self.B, self.N, self.C
        self.d = self.uni((B, N, C), -3, 3)
        self.jit = jitter_rows(self.rng, B, N, self.jit_pitch, self.shift, self.big)
        full = self.uni((B, self.d_bs), 5, 6)
        full.reshape(-1)[grid((B, self.d_bs), (N, self.d_pitch), (C, 1))] = self.d
        self.buf("d", full)
        self.buf("jitter", self.jit)
        t = self.buf("dsrc", None, torch.float32, B * self.dsrc_bs)
        self.tgt = grid((B, self.dsrc_bs), (N, self.dsrc_pitch), (C, 1))
        if L.load().aew_lc_scatter_needs_zero(N):           # the atomic form adds: its caller zeroes the target elements
            t[torch.from_numpy(GUARD + self.tgt.reshape(-1))] = 0

    def ops(self, ws):
        p = L.LcScatter()
        p.d, p.d_bs, p.d_pitch = P(ws, "d"), self.d_bs, self.d_pitch
        p.jitter, p.jit_pitch = P(ws, "jitter"), self.jit_pitch
        p.dsrc, p.dsrc_bs, p.dsrc_pitch = P(ws, "dsrc"), self.dsrc_bs, self.dsrc_pitch
        p.B, p.N, p.C, p.take_compat = self.B, self.N, self.C, self.take
        return [(L.OP_LC_SCATTER, p, "lc_scatter")]

    def expect(self):
        d = self.d.astype(np.float64)
        ref = R.lc_scatter(d, self.jit, self.take)
        S = R.lc_scatter(np.abs(d), self.jit, self.take)
        n = R.lc_scatter(np.ones_like(d), self.jit, self.take)
        out = []
        for cnt in np.unique(n):                             # one rule per number of terms
            m = n == cnt
            out.append(Expect("dsrc", self.tgt[m], ref[m], S[m], int(cnt), tag="lc_scatter"))
        return out


# =================================================================================================
class SpkCase(Case):
    """L = 3 layers (layer 1 without conv biases), C_lc = 8, 5 speakers of which speaker 2 is absent."""
    Lr, C_lc, n_speakers = 3, 8, 5

    def __init__(self, D, D_pad, G, B, spk_b=True, running=0, backward=False, split=False):
        self.D, self.D_pad, self.G, self.B, self.spk_b, self.running, self.backward, self.split = D, D_pad, G, B, spk_b, running, backward, split
        self.name = f"spk {'bwd' if backward else 'bias'} D{D}/{D_pad} G{G} B{B} spk_b={spk_b} running={running} split={split}"
        self.seed = 17 + D + G * 7 + B

    def fill(self):
        L_, D, G, B, Cc = self.Lr, self.D, self.G, self.B, self.C_lc + self.G
        off, o = {}, 5

        def take(name, n):
            nonlocal o
            off[name] = o
            o += n + 7                                           # 7 floats between tensors: never written
        take("spk_w", G * self.n_speakers)
        if self.spk_b:
            take("spk_b", G)
        for l in range(L_):
            for gate in (0, 1):
                if l != 1:
                    take(("b", gate, l), D)
                take(("p", gate, l), D * Cc)
        self.off, self.n_par = off, o
        self.off_bias = [[off.get(("b", g, l), -1) for l in range(L_)] for g in (0, 1)]
        self.off_proj = [[off[("p", g, l)] for l in range(L_)] for g in (0, 1)]
        self.off_spk_w, self.off_spk_b = off["spk_w"], off.get("spk_b", -1)
        self.params = self.uni((o,), -1, 1)
        self.voice = np.array([(0, 1, 3, 4)[(b * 7 // 3) % 4] for b in range(B)], dtype=np.int64)
        self.buf("params", self.params)
        self.buf("voice", self.voice)
        for n, tb in (("obs", self.off_bias[0]), ("obg", self.off_bias[1]), ("ops", self.off_proj[0]), ("opg", self.off_proj[1])):
            self.buf(n, np.array(tb, dtype=np.int64))
        self.args = (self.off_bias, self.off_proj, self.off_spk_w, self.off_spk_b, L_, D, self.D_pad, self.C_lc, G, self.n_speakers)
        _, gc = R.spk_bias(self.params, self.voice, *self.args)
        if not self.backward:
            self.buf("bias", None, torch.float32, B * L_ * 2 * self.D_pad)
            self.buf("gc", None, torch.float32, B * G)
            return
        self.gc = R.f32(gc)
        self.buf("gc", self.gc)
        cs = self.uni((B, L_, 2 * self.D_pad), -1, 1)
        if self.running:                                         # the first layers hold running sums over the batch
            cs[:, :self.running] = np.cumsum(cs[:, :self.running], axis=0, dtype=np.float32)
        self.colsum = cs
        self.buf("colsum", cs)
        g0 = self.uni((o,), -1, 1)                                # what the gradient buffer holds before the op
        g0[self.off_spk_w: self.off_spk_w + G * self.n_speakers].reshape(G, self.n_speakers)[:, 2] = 0.0
        if B > 16:                                               # several batch chunks ADD their bias / projection sums (aew_spk_bwd_t)
            for l in range(L_):
                for gate in (0, 1):
                    if self.off_bias[gate][l] >= 0:
                        g0[self.off_bias[gate][l]: self.off_bias[gate][l] + D] = 0
                    g0[self.off_proj[gate][l]: self.off_proj[gate][l] + D * Cc].reshape(D, Cc)[:, self.C_lc:] = 0
        self.g0 = g0
        self.buf("grads", g0)
        chunks = (B + 15) // 16
        for tag in ("a", "b"):
            self.buf("scratch_" + tag, None, torch.float32, L_ * 2 * chunks * 256)
            self.buf("tickets_" + tag, np.zeros(4, dtype=np.int32))

    def _common(self, ws, p):
        p.params, p.voice = P(ws, "params"), P(ws, "voice")
        p.off_bias_sig, p.off_bias_gate, p.off_proj_sig, p.off_proj_gate = P(ws, "obs"), P(ws, "obg"), P(ws, "ops"), P(ws, "opg")
        p.off_spk_w, p.off_spk_b = self.off_spk_w, self.off_spk_b
        p.B, p.L, p.D, p.D_pad, p.C_lc, p.G, p.n_speakers = self.B, self.Lr, self.D, self.D_pad, self.C_lc, self.G, self.n_speakers

    def ops(self, ws):
        if not self.backward:
            p = L.SpkBias()
            self._common(ws, p)
            p.bias, p.gc = P(ws, "bias"), P(ws, "gc")
            return [(L.OP_SPK_BIAS, p, "spk_bias")]
        out = []
        for tag, rng_ in (("a", (0, 1)), ("b", (1, 2))) if self.split else (("a", None),):
            p = L.SpkBwd()
            self._common(ws, p)
            p.colsum, p.gc, p.grads = P(ws, "colsum"), P(ws, "gc"), P(ws, "grads")
            p.colsum_running = self.running
            if rng_:
                p.layer_range = rng_[0] | (rng_[1] << 16)
            p.det_scratch, p.det_tickets = P(ws, "scratch_" + tag), P(ws, "tickets_" + tag)
            out.append((L.OP_SPK_BWD, p, "spk_bwd_" + tag))
        return out

    def regions(self):
        """{'bias_proj': indices of the bias / projection gradients the op writes, 'spk': the speaker rows (and bias) it adds into}"""
        D, G, Cc = self.D, self.G, self.C_lc + self.G
        bp = []
        for l in range(self.Lr):
            for gate in (0, 1):
                if self.off_bias[gate][l] >= 0:
                    bp.append(self.off_bias[gate][l] + np.arange(D))
                bp.append((self.off_proj[gate][l] + grid((D, Cc), (G, 1)) + self.C_lc).reshape(-1))
        present = np.unique(self.voice)
        spk = [(self.off_spk_w + grid((G, self.n_speakers)) + v).reshape(-1) for v in present]
        if self.spk_b:
            spk.append(self.off_spk_b + np.arange(G))
        return np.concatenate(bp), spk, present

    def expect(self):
        B, G, D, L_ = self.B, self.G, self.D, self.Lr
        if not self.backward:
            ref, gc = R.spk_bias(self.params, self.voice, *self.args)
            S, Sgc = R.spk_bias(np.abs(self.params), self.voice, *self.args)
            return [Expect("bias", np.arange(ref.size), ref, S, 2 * G + 1, tag="spk_bias"),
                    Expect("gc", np.arange(gc.size), gc, Sgc, 2, tag="spk_gc")]
        cs = R.spk_colsum_per_element(self.colsum, self.running)
        ref = R.spk_bwd(self.params, self.voice, *self.args, cs, self.gc, self.g0)
        S = R.spk_bwd(np.abs(self.params), self.voice, *self.args, np.abs(cs), np.abs(self.gc), np.abs(self.g0))
        bp, spk, present = self.regions()
        out = [Expect("grads", bp, ref[bp], S[bp], B, tag="spk_bwd_bias_proj")]
        for i, v in enumerate(present):
            out.append(Expect("grads", spk[i], ref[spk[i]], S[spk[i]], int((self.voice == v).sum()) * 2 * L_ * D + 1, tag="spk_bwd_emb"))
        if self.spk_b:
            out.append(Expect("grads", spk[-1], ref[spk[-1]], S[spk[-1]], B * 2 * L_ * D + 1, tag="spk_bwd_emb"))
        # the deterministic form's scratch and ticket are the op's own: whatever it leaves there is not an output
        # (the ticket word is back at zero, which the untouched rule holds bit for bit)
        for tag in ("a", "b"):
            n = self.len["scratch_" + tag]
            out.append(Expect("scratch_" + tag, np.arange(n), np.zeros(n), np.full(n, np.inf), tag="scratch"))
        return out


# =================================================================================================
class VqBwdCase(Case):
    K, codes = 9, (1, 4, 7)

    def __init__(self, Q, d, d_pitch, metric, demb=False, gmul=None):
        self.Q, self.d, self.d_pitch, self.metric, self.demb, self.gmul = Q, d, d_pitch, metric, demb, gmul
        self.name = f"vq_bwd Q{Q} d{d}/{d_pitch} metric{metric} demb={demb} gmul={gmul}"
        self.seed = 23 + Q + d
        self.coef, self.demb_coef = float(np.float32(0.25)), float(np.float32(0.7))

    def fill(self):
        Q, d, K = self.Q, self.d, self.K
        self.emb = self.uni((K, d), -1, 1)
        self.ind = np.array([self.codes[i % 3] for i in self.rng.integers(0, 3, Q)], dtype=np.int64)
        z = self.uni((Q, d), -1, 1)
        if Q == 1:
            z[0] = self.emb[self.ind[0]] if d == 16 else 0.0       # the one query: equal to its code, or the zero row
        else:
            z[0] = self.emb[self.ind[0]]                            # a query that equals its code row exactly (u == 0)
            z[1] = 0.0                                              # and the zero row (||z|| == 0)
        self.z, self.dzq = z, self.uni((Q, d), -1, 1)
        for n, a in (("ze", z), ("dzq", self.dzq)):
            full = self.uni((Q, self.d_pitch), 5, 6)
            full[:, :d] = a
            self.buf(n, full)
        self.buf("emb", self.emb)
        self.buf("ind", self.ind)
        self.buf("dze", None, torch.float32, Q * self.d_pitch)
        self.demb0 = self.uni((K, d), -1, 1)
        self.buf("demb", self.demb0)
        self.buf("gmul", np.array([self.gmul or 0.0] * 4, dtype=np.float32))

    def ops(self, ws):
        p = L.VqBwd()
        p.ze, p.emb, p.ind, p.dzq = P(ws, "ze"), P(ws, "emb"), P(ws, "ind"), P(ws, "dzq")
        p.Q, p.d, p.d_pitch, p.metric, p.coef, p.demb_coef = self.Q, self.d, self.d_pitch, self.metric, self.coef, self.demb_coef
        p.dze = P(ws, "dze")
        if self.demb:
            p.demb = P(ws, "demb")
        if self.gmul is not None:
            p.gmul = P(ws, "gmul")
        return [(L.OP_VQ_BWD, p, "vq_bwd")]

    def expect(self):
        Q, d = self.Q, self.d
        gm = None if self.gmul is None else float(np.float32(self.gmul))
        dze, demb = R.vq_bwd(self.z, self.emb, self.ind, self.dzq, self.metric, self.coef, self.demb_coef, gm,
                             self.demb0 if self.demb else None)
        t1, t2 = R.vq_bwd_terms(self.z, self.emb, self.ind, self.metric)
        S = np.abs(self.dzq.astype(np.float64)) + abs(self.coef * (gm or 1.0)) * (np.abs(t1) + np.abs(t2))
        idx = grid((Q, self.d_pitch), (self.d_pitch, 1))
        out = [Expect("dze", idx[:, :d], dze, S, 3, c=(2 * d + 16) if self.metric == 0 else 16, tag="vq_bwd_dze")]
        if self.d_pitch > d:
            out.append(Expect("dze", idx[:, d:], np.zeros((Q, self.d_pitch - d))))
        if self.demb:
            t = np.abs(self.z.astype(np.float64) - self.emb.astype(np.float64)[self.ind])
            for k in np.unique(self.ind):
                m = self.ind == k
                Sk = np.abs(self.demb0[k].astype(np.float64)) + abs(self.demb_coef * (gm or 1.0)) * 2.0 * t[m].sum(0)
                out.append(Expect("demb", k * d + np.arange(d), demb[k], Sk, int(m.sum()) + 1, tag="vq_bwd_demb"))
        return out


# =================================================================================================
class VaeCase(Case):
    free_nats = 2.0

    def __init__(self, Q, d, d_pitch, backward, kl_dev=False, gate=None, gmul=None):
        self.Q, self.d, self.d_pitch, self.backward, self.kl_dev, self.gate, self.gmul = Q, d, d_pitch, backward, kl_dev, gate, gmul
        self.name = f"vae Q{Q} d{d}/{d_pitch} {'bwd' if backward else 'fwd'} kl_dev={kl_dev} gate={gate} gmul={gmul}"
        self.seed = 29 + Q + d
        self.lin_pitch = 2 * d + 8
        self.kl_coef = float(np.float32(0.013))

    def fill(self):
        Q, d = self.Q, self.d
        self.mu, self.ls, self.eps = self.uni((Q, d), -2, 2), self.uni((Q, d), -3, 1.5), self.uni((Q, d), -2.5, 2.5)
        self.ds = self.uni((Q, d), -1, 1)
        lin = self.uni((Q, self.lin_pitch), 5, 6)
        lin[:, :d], lin[:, d:2 * d] = self.mu, self.ls
        self.buf("lin", lin)
        self.buf("eps", self.eps)
        full = self.uni((Q, self.d_pitch), 5, 6)
        full[:, :d] = self.ds
        self.buf("dsample", full)
        self.buf("sample", None, torch.float32, Q * self.d_pitch)
        self.buf("kl_terms", None, torch.float32, Q)
        self.buf("dlin", None, torch.float32, Q * self.lin_pitch)
        fn = np.float32(self.free_nats)
        self.kl_value = None if self.gate is None else float(np.nextafter(fn, np.float32(0 if self.gate == "below" else 4)))
        self.buf("kl_value", np.array([self.kl_value or 0.0] * 4, dtype=np.float32))
        self.kl_coef_dev = float(np.float32(0.021))
        self.buf("kl_coef_dev", np.array([self.kl_coef_dev] * 4, dtype=np.float32))
        self.buf("gmul", np.array([self.gmul or 0.0] * 4, dtype=np.float32))

    def ops(self, ws):
        p = L.Vae()
        p.lin, p.lin_pitch, p.eps = P(ws, "lin"), self.lin_pitch, P(ws, "eps")
        p.Q, p.d, p.d_pitch = self.Q, self.d, self.d_pitch
        p.sample, p.kl_terms, p.dsample, p.dlin = P(ws, "sample"), P(ws, "kl_terms"), P(ws, "dsample"), P(ws, "dlin")
        p.kl_coef, p.free_nats, p.backward = self.kl_coef, self.free_nats, int(self.backward)
        if self.gate is not None:
            p.kl_value = P(ws, "kl_value")
        if self.kl_dev:
            p.kl_coef_dev = P(ws, "kl_coef_dev")
        if self.gmul is not None:
            p.gmul = P(ws, "gmul")
        return [(L.OP_VAE, p, "vae")]

    def expect(self):
        Q, d = self.Q, self.d
        mu, ls, eps, ds = (a.astype(np.float64) for a in (self.mu, self.ls, self.eps, self.ds))
        sg = np.exp(0.5 * ls)
        # sigma = exp(ls / 2) carries (1 + |ls / 2|) 2^-24 relative (argument rounding + the function's own)
        rs = 1.0 + np.abs(0.5 * ls)
        if not self.backward:
            smp, kl = R.vae_fwd(mu, ls, eps)
            idx = grid((Q, self.d_pitch), (self.d_pitch, 1))
            out = [Expect("sample", idx[:, :d], smp, np.abs(mu) + np.abs(sg * eps) * rs, 2, tag="vae_sample"),
                   Expect("kl_terms", np.arange(Q), kl, (2.0 + 2.0 * rs + mu * mu + sg * sg * 2.0 * rs).sum(-1), 4 * d, tag="vae_kl")]
            if self.d_pitch > d:
                out.append(Expect("sample", idx[:, d:], np.zeros((Q, self.d_pitch - d))))
            return out
        gm = None if self.gmul is None else float(np.float32(self.gmul))
        k0 = self.kl_coef_dev if self.kl_dev else self.kl_coef
        dmu, dls = R.vae_bwd(mu, ls, eps, ds, k0, gm, self.kl_value, self.free_nats)
        k = abs(k0 * (gm or 1.0)) * (0.0 if (self.kl_value is not None and self.kl_value < self.free_nats) else 1.0)
        idx = grid((Q, self.lin_pitch), (2 * d, 1))
        return [Expect("dlin", idx[:, :d], dmu, np.abs(ds) + k * np.abs(mu), 2, tag="vae_dmu"),
                Expect("dlin", idx[:, d:], dls, np.abs(ds * eps * 0.5 * sg) * rs + k * 0.5 * (1.0 + sg * sg * 2.0 * rs), 3, tag="vae_dls")]


class AeNormCase(Case):
    def __init__(self, Q, d, d_pitch, backward, gmul=None):
        self.Q, self.d, self.d_pitch, self.backward, self.gmul = Q, d, d_pitch, backward, gmul
        self.name = f"ae_norm Q{Q} d{d}/{d_pitch} {'bwd' if backward else 'fwd'} gmul={gmul}"
        self.seed = 31 + Q + d
        self.coef = float(np.float32(0.6))

    def fill(self):
        Q, d = self.Q, self.d
        z = self.uni((Q, d), -1, 1)
        kinds = {16: 0, 64: 2, 100: 3}[d] if Q == 1 else None
        for q in range(Q):
            k = kinds if Q == 1 else q
            nrm = np.sqrt((z[q].astype(np.float64) ** 2).sum())
            if k == 0:
                z[q] = (z[q] * (0.5 / nrm)).astype(np.float32)            # norm < 1
            elif k == 1:
                z[q] = (z[q] * (1.7 / nrm)).astype(np.float32)            # norm > 1
            elif k == 2:
                z[q] = 0.0
                z[q, d // 3] = -1.0                                        # a unit basis vector: norm exactly 1
            elif k == 3:
                z[q] = 0.0                                                 # the zero row
        self.z, self.din = z, self.uni((Q, d), -1, 1)
        for n, a in (("ze", z), ("dze_in", self.din)):
            full = self.uni((Q, self.d_pitch), 5, 6)
            full[:, :d] = a
            self.buf(n, full)
        self.buf("term", None, torch.float32, Q)
        self.buf("dze", None, torch.float32, Q * self.d_pitch)
        self.buf("gmul", np.array([self.gmul or 0.0] * 4, dtype=np.float32))

    def ops(self, ws):
        p = L.AeNorm()
        p.ze, p.Q, p.d, p.d_pitch = P(ws, "ze"), self.Q, self.d, self.d_pitch
        p.term, p.dze_in, p.coef, p.dze, p.backward = P(ws, "term"), P(ws, "dze_in"), self.coef, P(ws, "dze"), int(self.backward)
        if self.gmul is not None:
            p.gmul = P(ws, "gmul")
        return [(L.OP_AE_NORM, p, "ae_norm")]

    def expect(self):
        Q, d = self.Q, self.d
        z = self.z.astype(np.float64)
        nrm = np.sqrt((z * z).sum(-1))
        if not self.backward:
            # d squares, a square root and a subtraction on S = ||z|| + 1
            return [Expect("term", np.arange(Q), R.ae_norm_fwd(z), nrm + 1.0, d + 2, tag="ae_norm_term")]
        gm = None if self.gmul is None else float(np.float32(self.gmul))
        ref = R.ae_norm_bwd(z, self.din, self.coef, gm)
        S = np.abs(self.din.astype(np.float64)) + np.abs(ref - self.din.astype(np.float64))
        idx = grid((Q, self.d_pitch), (self.d_pitch, 1))
        out = [Expect("dze", idx[:, :d], ref, S, 2, tag="ae_norm_dze")]
        if self.d_pitch > d:
            out.append(Expect("dze", idx[:, d:], np.zeros((Q, self.d_pitch - d))))
        return out


# =================================================================================================
# the case lists (the smallest shapes at which each branch of each kernel exists)
# =================================================================================================
SOFTMAX_SHAPES = [(256, 256, 256), (256, 256, 258), (64, 64, 64), (100, 128, 128), (16, 64, 64), (320, 320, 320)]


def softmax_cases():
    out = []
    for Q, Qp, pitch in SOFTMAX_SHAPES:
        reg = Q == 256 and Qp == 256 and pitch % 4 == 0
        out += [SoftmaxCase(Q, Qp, pitch, False, peak=reg), SoftmaxCase(Q, Qp, pitch, True), SoftmaxCase(Q, Qp, pitch, True, gmul=0.37)]
    return out


BASE_T = (1, 5, 16, 17, 67)
BASE_R = ((24, 32), (40, 40), (368, 384), (512, 512))


def base_gather_variants(T, R, R_pad):
    """[(case with Wt, the same case without)] over bias x one-hot"""
    return [(BaseGatherCase(T, R, R_pad, bias, oh, True), BaseGatherCase(T, R, R_pad, bias, oh, False))
            for bias in (True, False) for oh in (None, 256, 64)]


LC_SHAPES = [(B, N, C, Cp) for B in (1, 3, 5) for N in (1, 7, 29) for C, Cp in ((3, 8), (8, 16))]


def lc_cases(B, N, C, Cp):
    out = []
    for take in (0, 1):
        for shift in ((0, 1, 2) if B == 1 else (0,)):
            out += [LcGatherCase(B, N, C, Cp, take, shift), LcScatterCase(B, N, C, take, shift)]
    return out


def lc_big_cases():
    """N = 4096: the last size of the gather form (one case: every thread walks all N rows).  N = 4097: the atomic form."""
    return [LcScatterCase(1, 4096, 3, 0, big=True), LcScatterCase(2, 4097, 3, 0, big=True), LcScatterCase(2, 4097, 3, 1, big=True)]


SPK_SHAPES = [(D, Dp, G, B) for D, Dp in ((40, 48), (272, 272)) for G in (4, 16) for B in (1, 5, 16, 17, 33, 48)]
SPK_VARIANTS = [(True, 0), (False, 2), (True, 2), (False, 0)]          # (off_spk_b present, colsum_running)

VQ_SHAPES = [(Q, d, dp, m) for Q in (1, 5, 130) for d, dp in ((16, 16), (64, 64), (100, 128)) for m in (0, 1)]
VQ_VARIANTS = [(False, None), (True, 0.37), (True, None), (False, 0.37)]  # (demb set, gmul)

ROW_SHAPES = [(Q, d, dp) for Q in (1, 5) for d, dp in ((16, 16), (64, 64), (100, 128))]


def vae_cases(Q, d, dp):
    return [VaeCase(Q, d, dp, False),
            VaeCase(Q, d, dp, True), VaeCase(Q, d, dp, True, kl_dev=True, gmul=0.37),
            VaeCase(Q, d, dp, True, gate="below"), VaeCase(Q, d, dp, True, gate="above", gmul=0.37),
            VaeCase(Q, d, dp, True, kl_dev=True, gate="above"), VaeCase(Q, d, dp, True, kl_dev=True, gate="below", gmul=0.37)]


def ae_norm_cases(Q, d, dp):
    return [AeNormCase(Q, d, dp, False), AeNormCase(Q, d, dp, True), AeNormCase(Q, d, dp, True, gmul=0.37)]


def agree(case_a, after_a, case_b, after_b, coef=None, only=None, what=""):
    """Two runs of the same data (two kernel forms, two tunings, two layouts) against each other: exact elements bit for
    bit, the others within the rule of their expectation.  only: buffer names to compare."""
    ea = [e for e in case_a.expect() if only is None or e.buf in only]
    eb = [e for e in case_b.expect() if only is None or e.buf in only]
    assert [(e.buf, e.tag, e.idx.size) for e in ea] == [(e.buf, e.tag, e.idx.size) for e in eb], (what, "expectations differ")
    for a, b in zip(ea, eb):
        ga = after_a[a.buf][torch.from_numpy(GUARD + a.idx)]
        gb = after_b[b.buf][torch.from_numpy(GUARD + b.idx)]
        if a.S is None:
            assert torch.equal(_bits(ga), _bits(gb)), (what, a.buf, a.tag, "exact elements differ")
            continue
        k = coef[a.tag] if coef and a.tag in coef else (a.n + a.c) * U
        diff = np.abs(ga.double().numpy() - gb.double().numpy())
        bound = k * a.S + np.asarray(a.extra, dtype=np.float64) + TINY
        assert (diff <= bound).all(), (what, case_a.name, a.buf, a.tag, "forms disagree by", float((diff - bound).max()), "over the bound")


def same_bits(after_a, after_b, names, what=""):
    for n in names:
        assert torch.equal(_bits(after_a[n]), _bits(after_b[n])), (what, n, "not bit-identical")
