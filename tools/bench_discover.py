#!/usr/bin/env python3
"""AEW_OP_SEQ_DISCOVER at the sizes unit discovery has, in CELL UPDATES PER SECOND (one cell = one local distance and one
step of the dynamic programme), beside AEW_OP_SEQ_ALIGN's DTW and AEW_OP_SEQ_SEARCH on the SAME pairs in the SAME process:

  codes    P = 4096 pairs of 500 x 500 frames at D = 64     (utterance against utterance over code embeddings)
  cepstra  P = 4096 pairs of 1000 x 1000 frames at D = 12   (the same over static cepstra)
  lone     P = 1 pair of 1000 x 1000 at D = 12              (the latency of one pair: one wave on the whole device)

Method: the three op records are built once per case; `--warmup` launches of each, then `--repeats` (>= 7) rounds that
time one discover launch (sweep + pick, n_hits hits), one search launch and one DTW launch, each between two device
events on torch's current stream - the three alternate, so they see the same machine.  Median, minimum, maximum and
spread (max - min) of the launch time, cells/s at the median, and the ratios discover / dtw and search / dtw of the
rates.  The yardstick is the DTW kernel: discover does the same distance work, carries three more words per cell than
DTW (two more than search), keeps a running row maximum and stores five profile words per row, and runs the pick
(O(n_hits * n / 64) per pair).  The threshold sits a tenth under the typical distance of D normal channels, so that
alignments are born, live a while and die all over the matrix.  Nothing is asserted about speed: this is a record.

    timeout -k 10 900 python tools/bench_discover.py --out profiles/discover.txt
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CASES = {"codes": (4096, 500, 500, 64), "cepstra": (4096, 1000, 1000, 12), "lone": (1, 1000, 1000, 12)}
OPS = ("discover", "search", "dtw")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--n-hits", dest="n_hits", type=int, default=3)
    ap.add_argument("--cases", default="codes,cepstra,lone")
    ap.add_argument("--out", default="")
    return ap.parse_args()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_discover.py measures on the MI355X; no device found")
    if a.repeats < 7:
        sys.exit("at least 7 repeats")
    dev = torch.device("cuda", 0)
    import numpy as np
    from ae_wavenet_amd import _lib as L, align as AL
    L.load()
    props = torch.cuda.get_device_properties(0)
    out = ["AEW_OP_SEQ_DISCOVER - cell updates per second, beside AEW_OP_SEQ_ALIGN's DTW and AEW_OP_SEQ_SEARCH on the same pairs "
           "(tools/bench_discover.py)",
           "",
           f"box     : {props.name}, {getattr(props, 'gcnArchName', '')}, {props.multi_processor_count} CUs; torch {torch.__version__}, "
           f"HIP {getattr(torch.version, 'hip', None)}",
           f"method  : per case {a.warmup} warm-up launches of each op, then {a.repeats} rounds of one discover launch (sweep + pick, "
           f"n_hits = {a.n_hits}, min_len 1, band 0),",
           f"          one search launch (sweep + pick, n_hits = {a.n_hits}, rank mean) and one DTW launch over the same pairs, "
           "alternating, each between device",
           "          events; cells/s at the median launch time; ratios of the cells/s.  One cell = one local distance + one step.",
           "          threshold = 0.9 * sqrt(2 D), a tenth under the typical Euclidean distance of D normal channels.", ""]
    for name in a.cases.split(","):
        P, n, m, D = CASES[name]
        P = min(P, a.pairs)
        theta = 0.9 * math.sqrt(2.0 * D)
        gen = torch.Generator().manual_seed(len(name))
        xa, xb = torch.randn(P, n, D, generator=gen), torch.randn(P, m, D, generator=gen)
        ra = AL.Ragged(xa.to(dev).reshape(-1), [u * n * D for u in range(P)], [n] * P, D, 1, D)
        rb = AL.Ragged(xb.to(dev).reshape(-1), [u * m * D for u in range(P)], [m] * P, D, 1, D)
        pairs = AL.default_pairs(P, P, None)
        runs = {"discover": AL._DiscoverLaunch(L.ALIGN_EUCLID, theta, ra, rb, pairs, np.zeros(P, np.int64), a.n_hits, 1, 0),
                "search": AL._SearchLaunch(L.ALIGN_EUCLID, L.SEARCH_MEAN, ra, rb, pairs, a.n_hits, 1, 0),
                "dtw": AL._Launches(L.ALIGN_DTW, L.ALIGN_EUCLID, ra, rb, pairs, False, None)}
        for _ in range(a.warmup):
            for k in OPS:
                runs[k].run(name)
        torch.cuda.synchronize()
        ms = {k: [] for k in OPS}
        for _ in range(a.repeats):
            for k in OPS:
                ms[k].append(timed(lambda: runs[k].run(name)))
        cells = P * n * m
        rate = {}
        out.append(f"{name}: P = {P} pairs of {n} x {m}, D = {D}, threshold {theta:.4f}")
        for k in OPS:
            med = statistics.median(ms[k])
            rate[k] = cells / (med * 1e-3)
            out.append(f"  {k:8s} launch ms : " + " ".join(f"{x:.4f}" for x in ms[k]))
            out.append(f"  {k:8s} median / min / max / spread ms : {med:.4f} / {min(ms[k]):.4f} / {max(ms[k]):.4f} / "
                       f"{max(ms[k]) - min(ms[k]):.4f}   cell updates / s: {rate[k]:.4g}")
        disc = runs["discover"]
        found = int(disc.count.sum().item())
        out.append(f"  ratio discover / dtw : {rate['discover'] / rate['dtw']:.3f}   ratio search / dtw : {rate['search'] / rate['dtw']:.3f}   "
                   f"ratio discover / search : {rate['discover'] / rate['search']:.3f}")
        out.append(f"  (repeats found: {found} of {P * a.n_hits}, mean steps of hit 0: {float(disc.steps[:, 0].float().mean()):.1f}, "
                   f"pairs not finite: {int(disc.bad[0].item())})")
        out.append("")
        del runs, disc, ra, rb
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
