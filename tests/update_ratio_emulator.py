"""TEST INFRASTRUCTURE - the CPU plan interpreter with update / weight ratio tracking on top of the clipping interpreter
(tests/grad_clip_emulator.py): an Adam handler that honours aew_adam_t.track and a handler for AEW_OP_UPDATE_RATIO
(include/aewavenet.h semantics, torch CPU ops).  `emulate_uw` is `emulate_clip` with the engine's `ratio` plan patched as
well.  Not part of the product."""
import ctypes as C

import torch

from ae_wavenet_amd import _lib as L
from tests.grad_clip_emulator import ClipEmu


class RatioEmu(ClipEmu):
    def op_16(self, a):  # ADAM with aew_adam_t.track: the untracked step + per-chunk sums of (p_old - p_new)^2 and p_old^2
        if not a.track:
            return super().op_16(a)
        tr = C.cast(a.track, C.POINTER(L.UwTrack)).contents
        chunks = C.cast(tr.chunks_host, C.POINTER(L.UwChunk))
        part, poff = self.flat(tr.part)
        if tr.zero:
            part[poff:poff + 2 * tr.n_chunks] = 0
        idx = torch.arange(a.n)
        old = self.rd(a.p, idx).clone()
        track, a.track = a.track, None
        try:
            super().op_16(a)                                       # guard / clip skips included: then old == new
        finally:
            a.track = track
        new = self.rd(a.p, idx)
        lo, hi = tr.base, tr.base + a.n
        for c in range(tr.n_chunks):
            s, e = max(chunks[c].off, lo), min(chunks[c].off + chunks[c].len, hi)
            if s >= e:
                continue
            o, n = old[s - lo:e - lo], new[s - lo:e - lo]
            d = (o - n).double()                                   # the difference in fp32, the squares and sums in fp64
            part[poff + 2 * c] += (d * d).sum()
            part[poff + 2 * c + 1] += (o.double() * o.double()).sum()

    def op_27(self, p):  # UPDATE_RATIO: chunk sums -> per-tensor pairs (finalize = 0) or norms and ratio (finalize = 1)
        P = p.n_tensors
        tot = torch.zeros(2, P, dtype=torch.float64)
        if p.part:
            first = self.rd(p.first, torch.arange(P + 1))
            part, poff = self.flat(p.part)
            for t in range(P):
                seg = part[poff + 2 * int(first[t]):poff + 2 * int(first[t + 1])].view(-1, 2)
                tot[:, t] = seg.sum(0)
        if not p.finalize:
            self.wr(p.sums, torch.arange(2 * P), tot.reshape(-1))
            return
        if p.add_in:
            tot = tot + self.rd(p.add_in, torch.arange(2 * P)).view(2, P)
        if p.sums:
            self.wr(p.sums, torch.arange(2 * P), tot.reshape(-1))
        un, wn = tot[0].sqrt().float(), tot[1].sqrt().float()
        self.wr(p.out, torch.arange(3 * P), torch.cat([un, wn, un / wn]))


def emulate_uw(eng):
    """tests.plan_emulator.emulate with the tracking interpreter; eng.clip and eng.ratio are patched the way eng.opt is."""
    emu = RatioEmu(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "cb", "clip", "ratio"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
