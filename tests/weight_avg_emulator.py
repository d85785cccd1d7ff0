"""TEST INFRASTRUCTURE - the CPU plan interpreter with averaged weights on top of the tracking interpreter
(tests/update_ratio_emulator.py): an Adam handler that honours aew_adam_t.avg / avg_rate and a handler for AEW_OP_SWAP
(include/aewavenet.h semantics, torch CPU ops).  `emulate_avg` is `emulate_uw` with the engine's `swap` plan patched as
well.  Not part of the product."""
import numpy as np
import torch

from tests.update_ratio_emulator import RatioEmu


def avg_update(s, rate, p_new):
    """The kernel's three fp32 roundings, s + rate * (p_new - s), on numpy float32 arrays."""
    s, p_new, rate = np.asarray(s, np.float32), np.asarray(p_new, np.float32), np.float32(rate)
    return (s + rate * (p_new - s)).astype(np.float32)


class AvgEmu(RatioEmu):
    def op_16(self, a):  # ADAM with aew_adam_t.avg: the step without it, then avg += avg_rate * (p_new - avg) over its range
        if not a.avg:
            return super().op_16(a)
        assert 0.0 <= a.avg_rate <= 1.0
        skipped = self._guarded(a) or (bool(a.clip) and float(self.rd(a.clip, torch.arange(2))[1]) != 0.0)
        avg, a.avg = a.avg, None
        try:
            super().op_16(a)
        finally:
            a.avg = avg
        if skipped:                                                 # a step the device skips leaves the average alone
            return
        n = torch.arange(a.n)
        new = avg_update(self.rd(a.avg, n).numpy(), a.avg_rate, self.rd(a.p, n).numpy())
        self.wr(a.avg, n, torch.from_numpy(new))

    def op_28(self, p):  # SWAP: a[i] <-> b[i]
        n = torch.arange(p.n)
        x, y = self.rd(p.a, n).clone(), self.rd(p.b, n).clone()
        self.wr(p.a, n, y); self.wr(p.b, n, x)


def emulate_avg(eng):
    """tests.plan_emulator.emulate with the averaging interpreter; eng.clip, eng.ratio and eng.swap are patched the way
    eng.opt is."""
    emu = AvgEmu(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "cb", "clip", "ratio", "swap"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
