"""TEST INFRASTRUCTURE - the CPU plan interpreter with parameter groups on top of the averaging interpreter
(tests/weight_avg_emulator.py): a handler for AEW_OP_ADAM_GROUPS (aew_adam_grouped_t; include/aewavenet.h semantics: per-tensor
lr, decoupled decay as ONE numpy fp32 multiply in front of the step, frozen tensors left alone).  `emulate_groups` is
`emulate_avg` with this interpreter.  Not part of the product."""
import ctypes as C

import numpy as np
import torch

from ae_wavenet_amd import _lib as L
from tests.weight_avg_emulator import AvgEmu


class GroupsEmu(AvgEmu):
    def op_37(self, op):  # ADAM_GROUPS: chunk by chunk, the Adam step without a record on (p * decay_t) with lr_t
        a = op.adam
        assert op.groups
        gr = C.cast(op.groups, C.POINTER(L.AdamGroups)).contents
        chunks = C.cast(gr.chunks_host, C.POINTER(L.UwChunk))
        assert gr.base % 4 == 0 and gr.n_chunks >= 1 and gr.tensors
        tbl = self.rd(gr.tensors, torch.arange(4 * gr.n_tensors)).to(torch.int32).numpy().reshape(-1, 4)
        lrs, decays, frozen = tbl[:, 0].copy().view(np.float32), tbl[:, 1].copy().view(np.float32), tbl[:, 2]
        lo, hi = gr.base, gr.base + a.n
        tr = C.cast(a.track, C.POINTER(L.UwTrack)).contents if a.track else None
        part = None
        if tr is not None:
            assert tr.base == gr.base and tr.n_chunks == gr.n_chunks
            part, poff = self.flat(tr.part)
            if tr.zero:
                part[poff:poff + 2 * tr.n_chunks] = 0
        skipped = self._guarded(a) or (bool(a.clip) and float(self.rd(a.clip, torch.arange(2))[1]) != 0.0)
        keep = (a.p, a.g, a.m, a.v, a.avg, a.n, a.lr, a.track)
        covered = 0
        try:
            for c in range(gr.n_chunks):
                # this launch's part of the chunk, pad elements behind it included: [s, e_pad) is updated, [s, e) summed
                off, ln, t = chunks[c].off, chunks[c].len, chunks[c].tensor
                s, e, e_pad = max(off, lo), min(off + ln, hi), min(off + (ln + 3) // 4 * 4, hi)
                if s >= e_pad:
                    continue
                assert 0 <= t < gr.n_tensors
                covered += e_pad - s
                idx = torch.arange(e_pad - s)
                p_ptr = keep[0] + 4 * (s - lo)
                old = self.rd(p_ptr, idx).clone()
                if not frozen[t] and not skipped:
                    if decays[t] != np.float32(1.0):
                        self.wr(p_ptr, idx, torch.from_numpy(old.numpy() * decays[t]))      # one fp32 rounding
                    a.p, a.g, a.m, a.v = (x + 4 * (s - lo) for x in keep[:4])
                    a.avg = keep[4] + 4 * (s - lo) if keep[4] else None
                    a.n, a.lr, a.track = e_pad - s, float(lrs[t]), None
                    self.op_16(a)
                if part is not None and e > s:
                    o, n = old[:e - s], self.rd(p_ptr, idx)[:e - s]
                    d = (o - n).double()                           # p_old is the value in front of the decay
                    part[poff + 2 * c] += (d * d).sum()
                    part[poff + 2 * c + 1] += (o.double() * o.double()).sum()
        finally:
            a.p, a.g, a.m, a.v, a.avg, a.n, a.lr, a.track = keep
        assert covered == a.n, "the chunks (+ pads) must cover the launch's range"


def emulate_groups(eng, emu_cls=None):
    """tests.plan_emulator.emulate with the grouping interpreter (or a subclass of it); eng.opt_groups, eng.clip, eng.ratio,
    eng.swap, eng.restart and eng.accum are patched the way eng.opt is."""
    emu = (emu_cls or GroupsEmu)(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "opt_groups", "cb", "clip", "ratio", "swap", "restart", "accum"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
