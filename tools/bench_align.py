#!/usr/bin/env python3
"""AEW_OP_SEQ_ALIGN at the sizes its callers have, in CELL UPDATES PER SECOND (one cell = one local distance and one
step of the dynamic programme):

  dtw_codes    P = 4096 pairs of 500 x 500 frames at D = 64   (code embeddings, 10 s at 50 Hz)
  dtw_cepstra  P = 4096 pairs of 1000 x 1000 frames at D = 12 (cepstra)
  dtw_lone     P = 1 pair of 1000 x 1000 at D = 12            (the latency of a lone pair)
  edit         P = 4096 pairs of 500 x 500 symbols

Method: the op record is built once; per case `--warmup` launches, then `--repeats` (>= 7) timed launches, each between
two device events on torch's current stream; median, minimum, maximum and the spread (max - min) of the launch time are
reported, and cells/s at the median.  Two figures stand beside each case, named for what they are:

  torch_cpu_antidiagonal   the emulator's rule (tests/seq_align_emulator.py) as a torch CPU implementation that takes one
                           anti-diagonal of ALL its pairs at a time, at 16 threads, on the first `--cpu-pairs` pairs of the
                           same inputs (wall clock, one run after one warm-up run on a tenth of the pairs);
  valu_bound               cells/s if nothing but the cell's own fp32 operations were issued at the vector peak of the
                           part: (3 D subtract / multiply / add + 1 square root + 8 for the three-way minimum, the sum
                           and the step count) operations per cell over 157.3e12 fp32 operations per second
                           (MI355X vector peak).  No kernel built from unfused operations reaches it - the peak counts
                           a fused multiply-add as two - it is a ceiling, not a target.

One JSON line on stdout, also written to --out.  Nothing is asserted about speed: this is a record.

    timeout -k 10 900 python tools/bench_align.py --out profiles/align.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

VECTOR_PEAK_FP32 = 157.3e12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--cpu-pairs", dest="cpu_pairs", type=int, default=32)
    ap.add_argument("--cases", default="dtw_codes,dtw_cepstra,dtw_lone,edit")
    ap.add_argument("--out", default="")
    return ap.parse_args()


def cpu_dtw_antidiagonal(a, b):
    """a (P, n, D), b (P, m, D) fp32 CPU tensors -> cost (P,): the rule, one anti-diagonal of every pair at a time."""
    P, n, D = a.shape
    m = b.shape[1]
    acc = torch.zeros(P, n, m)
    for k in range(D):
        t = a[:, :, k, None] - b[:, None, :, k]
        acc = acc + t * t
    d = acc.double().sqrt().float()        # correctly rounded (torch's vectorised fp32 sqrt on the CPU is not, in the last bit)
    inf = float("inf")
    Cm = torch.full((P, n + 1, m + 1), inf)                   # one border row / column of +inf: the missing predecessors
    for s in range(n + m - 1):
        i = torch.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        if s == 0:
            Cm[:, 1, 1] = d[:, 0, 0]
            continue
        cd, cu, cl = Cm[:, i, j], Cm[:, i, j + 1], Cm[:, i + 1, j]
        best = torch.where(cu < cd, cu, cd)
        best = torch.where(cl < best, cl, best)
        Cm[:, i + 1, j + 1] = d[:, i, j] + best
    return Cm[:, n, m]


def cpu_edit_antidiagonal(a, b):
    P, n = a.shape
    m = b.shape[1]
    E = torch.zeros(P, n + 1, m + 1, dtype=torch.int32)
    E[:, :, 0] = torch.arange(n + 1, dtype=torch.int32)
    E[:, 0, :] = torch.arange(m + 1, dtype=torch.int32)
    for s in range(n + m - 1):
        i = torch.arange(max(0, s - m + 1), min(n - 1, s) + 1)
        j = s - i
        sub = E[:, i, j] + (a[:, i] != b[:, j]).to(torch.int32)
        E[:, i + 1, j + 1] = torch.minimum(sub, torch.minimum(E[:, i, j + 1], E[:, i + 1, j]) + 1)
    return E[:, n, m]


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_align.py measures on the MI355X; no device found")
    if a.repeats < 7:
        sys.exit("at least 7 repeats")
    dev = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, align as AL
    L.load()
    torch.set_num_threads(16)
    cases = {"dtw_codes": ("dtw", a.pairs, 500, 64), "dtw_cepstra": ("dtw", a.pairs, 1000, 12),
             "dtw_lone": ("dtw", 1, 1000, 12), "edit": ("edit", a.pairs, 500, 1)}
    props = torch.cuda.get_device_properties(0)
    rec = {"what": "AEW_OP_SEQ_ALIGN: cell updates per second", "cases": {},
           "method": f"{a.warmup} warm-up launches, {a.repeats} timed launches between device events, per case; cells/s at "
                     "the median launch time",
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
                   "torch": torch.__version__, "hip": getattr(torch.version, "hip", None), "cpu_threads": torch.get_num_threads()}}
    for name in a.cases.split(","):
        kind, P, n, D = cases[name]
        gen = torch.Generator().manual_seed(len(name))
        if kind == "dtw":
            xa, xb = torch.randn(P, n, D, generator=gen), torch.randn(P, n, D, generator=gen)
            ra = AL.Ragged(xa.to(dev).reshape(-1), [u * n * D for u in range(P)], [n] * P, D, 1, D)
            rb = AL.Ragged(xb.to(dev).reshape(-1), [u * n * D for u in range(P)], [n] * P, D, 1, D)
            run = AL._Launches(L.ALIGN_DTW, L.ALIGN_EUCLID, ra, rb, AL.default_pairs(P, P, None), False, None)
            ops_per_cell = 3 * D + 1 + 8
        else:
            xa, xb = torch.randint(0, 64, (P, n), generator=gen), torch.randint(0, 64, (P, n), generator=gen)
            ra = AL.Ragged(xa.to(dev).reshape(-1), [u * n for u in range(P)], [n] * P, 1, 1, 1)
            rb = AL.Ragged(xb.to(dev).reshape(-1), [u * n for u in range(P)], [n] * P, 1, 1, 1)
            run = AL._Launches(L.ALIGN_EDIT, 0, ra, rb, AL.default_pairs(P, P, None), False, None)
            ops_per_cell = None
        for _ in range(a.warmup):
            run.run(name)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run.run(name)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        cells = P * n * n
        med = statistics.median(ms)
        # the same rule on the CPU, on the first pairs of the same inputs
        cp = max(1, min(a.cpu_pairs, P))
        fn = cpu_dtw_antidiagonal if kind == "dtw" else cpu_edit_antidiagonal
        fn(xa[:max(1, cp // 10)], xb[:max(1, cp // 10)])
        t0 = time.perf_counter()
        ref = fn(xa[:cp], xb[:cp])
        cpu_s = time.perf_counter() - t0
        got = (run.cost if kind == "dtw" else run.steps)[:cp].cpu()
        case = {"pairs": P, "n": n, "m": n, "D": D, "launch_ms": [round(x, 4) for x in ms], "median_ms": round(med, 4),
                "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4),
                "cells_per_s": round(cells / (med * 1e-3)),
                "torch_cpu_antidiagonal": {"pairs": cp, "threads": torch.get_num_threads(), "seconds": round(cpu_s, 3),
                                           "cells_per_s": round(cp * n * n / cpu_s),
                                           "same_result_as_device": bool(torch.equal(ref.to(got.dtype), got))}}
        if ops_per_cell is not None:
            case["valu_bound"] = {"ops_per_cell": ops_per_cell, "peak_fp32_ops_per_s": VECTOR_PEAK_FP32,
                                  "cells_per_s": round(VECTOR_PEAK_FP32 / ops_per_cell)}
            case["fraction_of_valu_bound"] = round(case["cells_per_s"] / case["valu_bound"]["cells_per_s"], 4)
        rec["cases"][name] = case
        del run, ra, rb
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
