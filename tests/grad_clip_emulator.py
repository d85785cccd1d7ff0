"""TEST INFRASTRUCTURE - the CPU plan interpreter (tests/plan_emulator.py) with gradient clipping: a handler for
AEW_OP_GRAD_NORM and an Adam handler that honours aew_adam_t.clip (include/aewavenet.h semantics, torch CPU ops).
`emulate_clip` is `emulate` with the engine's `clip` plan patched as well.  Not part of the product."""
import math

import torch

from ae_wavenet_amd import _lib as L
from tests.plan_emulator import Emu


class ClipEmu(Emu):
    def op_26(self, p):  # GRAD_NORM: fp64 sum of squares over the ranges (+ add_in), then norm / coefficient / flag / count
        assert 1 <= p.n_ranges <= L.GRAD_NORM_MAX_RANGES
        total = torch.zeros((), dtype=torch.float64)
        for i in range(p.n_ranges):
            if p.n[i] > 0:
                x = self.rd(p.x[i], torch.arange(p.n[i])).double()
                total = total + (x * x).sum()
        if p.add_in:
            total = total + self.rd(p.add_in, torch.arange(1))[0]
        self.wr(p.sumsq, torch.arange(1), total.reshape(1))
        if not p.finalize or self._guarded(p):
            return
        norm = float(total.sqrt()) * abs(p.grad_scale)
        nf = float(torch.tensor(norm, dtype=torch.float32))
        o = self.rd(p.out, torch.arange(4)).clone()
        if not math.isfinite(float(total)):
            o[0], o[1], o[2], o[3] = nf, 0.0, 1.0, o[3] + 1.0
        else:
            coef = 1.0 if nf <= p.max_norm else min(1.0, float(torch.tensor(p.max_norm / (norm + p.eps), dtype=torch.float32)))
            o[0], o[1], o[2] = nf, coef, 0.0
        self.wr(p.out, torch.arange(4), o)

    def op_16(self, a):  # ADAM with aew_adam_t.clip: clip[1] != 0 -> no-op, else g * grad_scale * clip[0]
        if not a.clip:
            return super().op_16(a)
        if self._guarded(a):
            return
        clip = self.rd(a.clip, torch.arange(2))
        if float(clip[1]) != 0.0:
            return
        n = torch.arange(a.n)
        p, g, m, v = (self.rd(x, n) for x in (a.p, a.g, a.m, a.v))
        g = g * a.grad_scale * clip[0]
        m = a.beta1 * m + (1 - a.beta1) * g
        v = a.beta2 * v + (1 - a.beta2) * g * g
        p = p - (a.lr / a.bc1) * m / (v.sqrt() / (a.bc2 ** 0.5) + a.eps)
        self.wr(a.p, n, p); self.wr(a.m, n, m); self.wr(a.v, n, v)


def emulate_clip(eng):
    """tests.plan_emulator.emulate with the clipping interpreter; eng.clip is patched the way eng.opt is."""
    emu = ClipEmu(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "cb", "clip"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
