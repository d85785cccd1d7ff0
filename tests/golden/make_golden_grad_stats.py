#!/usr/bin/env python3
"""Generate tests/golden/grad_stats.npz by IMPORTING the reference's grad_analysis.py, unmodified.

Runs only in the build container (needs the reference checkout, which never travels to the GPU box).  Everything written
is data: a recorded gradient sequence, the running statistics and the quantiles the reference's functions produced for
it, and the argument names of those functions.  Re-run with

    python -B tests/golden/make_golden_grad_stats.py

A tiny nn.Module with four parameters of 1, 3, 4 and 4099 elements; the closure sets .grad from the recorded sequence and
leaves the 3-element parameter's grad None.  The 4-element tensor's sequence is constant from sample 1 on and chosen
(by a seed search) so that the reference's count convention leaves a negative s at b = 1 that survives to the end: the
fixture then holds a NaN quantile that came from the reference itself.
"""
import inspect
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get("AEW_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch

sys.path.insert(0, REF)
import grad_analysis as GA      # noqa: E402

N_BATCH = 5
QUANTILES = [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1]
SHAPES = {"a": (1,), "b": (3,), "c": (2, 2), "d": (4099,)}
NO_GRAD = "b"


class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        for n, shp in SHAPES.items():
            setattr(self, n, torch.nn.Parameter(torch.zeros(shp)))


def run_reference(seq):
    """mu / s after every step through mu_s_incr (the reference's own loop, restated call for call), and grad_stats."""
    mu, s, mus, ss = {}, {}, {}, {}
    for n in seq:
        mu[n] = s[n] = None
        mus[n], ss[n] = [], []
    for b in range(N_BATCH):
        for n in seq:
            mu[n], s[n] = GA.mu_s_incr(torch.from_numpy(seq[n][b + 1]), b, mu[n], s[n])
            mus[n].append(mu[n].numpy().copy())
            ss[n].append(s[n].numpy().copy())
    model = Tiny()
    calls = [0]

    def closure():
        i = calls[0]
        calls[0] += 1
        for n, p in model.named_parameters():
            p.grad = None if n == NO_GRAD else torch.from_numpy(seq[n][i]).reshape(SHAPES[n]).clone()

    quant = GA.grad_stats(model, closure, N_BATCH, QUANTILES)
    assert calls[0] == N_BATCH + 1
    return mus, ss, quant


def main():
    seed = 0
    rs = np.random.RandomState(seed)
    seq = {n: rs.standard_normal((N_BATCH + 1, int(np.prod(SHAPES[n])))).astype(np.float32)
           for n in SHAPES if n != NO_GRAD}
    # the constant tensor: two of its four (sample 0, sample 1) pairs are the first of 200 000 random pairs whose s is
    # negative after b = 1 under the reference's count convention
    x0, x1 = rs.standard_normal((2, 200000)).astype(np.float32)
    mu1, s1 = GA.mu_s_incr(torch.from_numpy(x1), 1, torch.from_numpy(x0), torch.zeros(200000))
    neg = np.nonzero(s1.numpy() < 0)[0][:2]
    assert len(neg) == 2
    seq["c"][1, :2], seq["c"][2, :2] = x0[neg], x1[neg]  # (entry 0 of a sequence is the closure call that only selects)
    seq["c"][3:] = seq["c"][2]
    mus, ss, quant = run_reference(seq)
    assert (ss["c"][-1] < 0).sum() >= 2
    out = {"seed": np.int64(seed), "n_batch": np.int64(N_BATCH), "quantiles": np.asarray(QUANTILES, np.float64),
           "names": np.asarray(list(SHAPES)), "no_grad": np.asarray(NO_GRAD),
           "shapes": np.asarray([",".join(map(str, SHAPES[n])) for n in SHAPES])}
    for n in seq:
        out["seq_" + n] = seq[n]
        out["mu_" + n] = np.stack(mus[n])
        out["s_" + n] = np.stack(ss[n])
        out["quant_" + n] = np.asarray(quant[n], np.float32)
        assert all(np.float32(v) == v or v != v for v in quant[n])
    assert np.isnan(out["quant_c"]).any(), "the constant tensor's negative s gives a NaN quantile"
    for fn in ("mu_s_incr", "quantiles", "grad_stats"):
        out["args_" + fn] = np.asarray(list(inspect.signature(getattr(GA, fn)).parameters))
    np.savez_compressed(os.path.join(HERE, "grad_stats.npz"), **out)
    print("seed", seed, {n: out["quant_" + n] for n in seq})


if __name__ == "__main__":
    main()
