"""TEST INFRASTRUCTURE - the restart of dead codes (aew_vq_restart_t, include/aewavenet.h) restated in numpy, and the
CPU plan interpreter with a handler for it on top of the averaging interpreter (tests/weight_avg_emulator.py).
`restart_reference` is the rule itself: the hash through oracle.jitter_rng.mix64, the arithmetic in np.float32, the
coprime search through math.gcd.  `emulate_restart` is `emulate_avg` with the engine's `restart` plan patched as well.
Not part of the product."""
import math

import numpy as np
import torch

from oracle.jitter_rng import mix64
from tests.weight_avg_emulator import AvgEmu

_M = (1 << 64) - 1
_G = 0x9e3779b97f4a7c15


def restart_ab(Q, seed, call):
    """(a, b) of the row rule q_r = (a + r * b) % Q, as Python integers."""
    with np.errstate(over="ignore"):
        h = mix64(mix64(np.uint64((seed + _G) & _M)) ^ np.uint64((call + _G) & _M))
        a = int(mix64(h ^ np.uint64(1))) % Q
        if Q == 1:
            return a, 1
        b0 = int(mix64(h ^ np.uint64(2))) % (Q - 1)
    i = 0
    while True:
        c = 1 + (b0 + i) % (Q - 1)
        if math.gcd(c, Q) == 1:
            return a, c
        i += 1


def restart_rows(Q, n, seed, call):
    a, b = restart_ab(Q, seed, call)
    return [(a + r * b) % Q for r in range(n)]


def restart_reference(ze, emb, numer, denom, max_codes, min_usage, denom_init, seed, call, total=0):
    """ze [Q][d_pitch], emb [K][d], numer [K][d], denom [K] (float32 arrays, not modified) ->
    (emb, numer, denom, out int32 [4], pairs int32 [max_codes][2]) after one launch; `total` is out[2] before it."""
    ze, emb, numer, denom = (np.array(x, dtype=np.float32) for x in (ze, emb, numer, denom))
    Q, (K, d) = ze.shape[0], emb.shape
    assert ze.shape[1] >= d and numer.shape == (K, d) and denom.shape == (K,)
    mu, di = np.float32(min_usage), np.float32(denom_init)
    with np.errstate(invalid="ignore"):
        dead = [k for k in range(K) if not (denom[k] >= mu)]
    n = min(len(dead), Q, max_codes)
    rows = restart_rows(Q, n, seed, call)
    pairs = np.full((max_codes, 2), -1, np.int32)
    for r, (k, q) in enumerate(zip(dead[:n], rows)):
        numer[k] = ze[q, :d] * di
        emb[k] = numer[k] / di
        denom[k] = di
        pairs[r] = (k, q)
    return emb, numer, denom, np.array([len(dead), n, total + n, 0], np.int32), pairs


class RestartEmu(AvgEmu):
    def op_29(self, p):  # VQ_RESTART
        if self._guarded(p):
            return
        assert p.Q >= 1 and p.K >= 1 and 1 <= p.d <= p.d_pitch and 1 <= p.max_codes <= 1024
        kd, k = torch.arange(p.K * p.d), torch.arange(p.K)
        ze = self.rd(p.ze, torch.arange(p.Q * p.d_pitch)).numpy().reshape(p.Q, p.d_pitch)
        total = int(self.rd(p.out, torch.arange(4))[2])
        emb, numer, denom, out, pairs = restart_reference(
            ze, self.rd(p.emb, kd).numpy().reshape(p.K, p.d), self.rd(p.numer, kd).numpy().reshape(p.K, p.d),
            self.rd(p.denom, k).numpy(), p.max_codes, p.min_usage, p.denom_init, p.seed, p.call, total)
        for kk in pairs[:int(out[1]), 0].tolist():               # only the restarted rows are written
            row = kk * p.d + torch.arange(p.d)
            self.wr(p.emb, row, torch.from_numpy(emb[kk]))
            self.wr(p.numer, row, torch.from_numpy(numer[kk]))
            self.wr(p.denom, torch.tensor([kk]), torch.from_numpy(denom[kk:kk + 1]))
        self.wr(p.out, torch.arange(4), torch.from_numpy(out))
        if p.pairs:
            self.wr(p.pairs, torch.arange(2 * p.max_codes), torch.from_numpy(pairs.reshape(-1)))


def emulate_restart(eng):
    """tests.plan_emulator.emulate with the restarting interpreter; eng.clip, eng.ratio, eng.swap and eng.restart are
    patched the way eng.opt is."""
    emu = RestartEmu(eng.ws)
    eng._stream = lambda: 0
    eng._run = lambda plan, timing=False: emu.run(plan)
    for name in ("opt", "cb", "clip", "ratio", "swap", "restart"):
        pl = getattr(eng, name, None)
        if pl is not None:
            pl.run = (lambda p: (lambda stream=0: emu.run(p)))(pl)
    return eng
