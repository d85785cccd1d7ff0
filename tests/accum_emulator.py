"""TEST INFRASTRUCTURE - the CPU plan interpreter with a handler for AEW_OP_ACCUM (aew_accum_t, include/aewavenet.h) on top
of the restarting interpreter (tests/code_restart_emulator.py), in numpy fp32: one round-to-nearest addition per element.
`fold` is the rule itself; `emulate_accum` is `emulate_restart` with the engine's `accum` plan patched as well.  Not part of
the product."""
import numpy as np
import torch

from tests.code_restart_emulator import RestartEmu

FIRST, ADD, LAST = 0, 1, 2


def fold(acc, g, mode):
    """(acc', g') after one launch on float32 arrays (not modified)."""
    acc, g = np.array(acc, np.float32), np.array(g, np.float32)
    assert mode in (FIRST, ADD, LAST) and acc.shape == g.shape
    if mode == FIRST:
        return g.copy(), g
    with np.errstate(all="ignore"):
        s = (acc + g).astype(np.float32)
    return (s, g) if mode == ADD else (acc, s)


def sequential_sum(gs):
    """((g1 + g2) + g3) + ... in fp32: what .grad holds after the last backward of a group."""
    s = np.array(gs[0], np.float32)
    for g in gs[1:]:
        with np.errstate(all="ignore"):
            s = (s + np.asarray(g, np.float32)).astype(np.float32)
    return s


class AccumEmu(RestartEmu):
    def op_34(self, p):  # ACCUM
        assert p.n >= 0 and p.mode in (FIRST, ADD, LAST)
        if p.n == 0:
            return
        n = torch.arange(p.n)
        acc, g = fold(self.rd(p.acc, n).numpy(), self.rd(p.g, n).numpy(), p.mode)
        if p.mode == LAST:
            self.wr(p.g, n, torch.from_numpy(g))
        else:
            self.wr(p.acc, n, torch.from_numpy(acc))


def emulate_accum(eng, emu_cls=AccumEmu):
    """tests.plan_emulator.emulate with the accumulating interpreter (or a subclass of it); eng.clip, eng.ratio, eng.swap,
    eng.restart and eng.accum are patched the way eng.opt is."""
    emu = emu_cls(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "cb", "clip", "ratio", "swap", "restart", "accum"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
