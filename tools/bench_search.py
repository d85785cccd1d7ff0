#!/usr/bin/env python3
"""AEW_OP_SEQ_SEARCH at the sizes its callers have, in CELL UPDATES PER SECOND (one cell = one local distance and one
step of the dynamic programme), beside AEW_OP_SEQ_ALIGN's DTW on the SAME pairs in the SAME process:

  word_codes    P = 4096 pairs of 32 x 1000 frames at D = 64    (a word in an utterance, over code embeddings; a 32-row
                                                                 query uses HALF the lanes of its wave)
  word_cepstra  P = 4096 pairs of 64 x 1000 frames at D = 12
  phrase        P = 4096 pairs of 200 x 1000 frames at D = 12   (four strips of 64 query rows: the boundary rows go
                                                                 through the workspace)
  lone          P = 1 pair of 64 x 100000 at D = 12             (the latency of one long document)

Method: both op records are built once per case; `--warmup` launches of each, then `--repeats` (>= 7) rounds that time
one search launch (sweep + pick, n_hits hits) and then one DTW launch, each between two device events on torch's current
stream - the two alternate, so they see the same machine.  Median, minimum, maximum and spread (max - min) of the launch
time, cells/s at the median, and the ratio search / dtw of the two rates.  The yardstick is the DTW kernel: search does
the same distance work, carries one more value per cell, stores three profile words per column and runs the pick
(O(n_hits * m / 64) per pair).  Nothing is asserted about speed: this is a record.

    timeout -k 10 900 python tools/bench_search.py --out profiles/search.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CASES = {"word_codes": (4096, 32, 1000, 64), "word_cepstra": (4096, 64, 1000, 12), "phrase": (4096, 200, 1000, 12),
         "lone": (1, 64, 100000, 12)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--n-hits", dest="n_hits", type=int, default=3)
    ap.add_argument("--cases", default="word_codes,word_cepstra,phrase,lone")
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
        sys.exit("bench_search.py measures on the MI355X; no device found")
    if a.repeats < 7:
        sys.exit("at least 7 repeats")
    dev = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, align as AL
    L.load()
    props = torch.cuda.get_device_properties(0)
    out = ["AEW_OP_SEQ_SEARCH - cell updates per second, beside AEW_OP_SEQ_ALIGN's DTW on the same pairs (tools/bench_search.py)",
           "",
           f"box     : {props.name}, {getattr(props, 'gcnArchName', '')}, {props.multi_processor_count} CUs; torch {torch.__version__}, "
           f"HIP {getattr(torch.version, 'hip', None)}",
           f"method  : per case {a.warmup} warm-up launches of each op, then {a.repeats} rounds of one search launch (sweep + pick, "
           f"n_hits = {a.n_hits}, rank mean)",
           "          and one DTW launch over the same pairs, alternating, each between device events; cells/s at the median",
           "          launch time; ratio = search cells/s over dtw cells/s.  One cell = one local distance + one step.", ""]
    for name in a.cases.split(","):
        P, n, m, D = CASES[name]
        P = min(P, a.pairs)
        gen = torch.Generator().manual_seed(len(name))
        xq, xd = torch.randn(P, n, D, generator=gen), torch.randn(P, m, D, generator=gen)
        rq = AL.Ragged(xq.to(dev).reshape(-1), [u * n * D for u in range(P)], [n] * P, D, 1, D)
        rd = AL.Ragged(xd.to(dev).reshape(-1), [u * m * D for u in range(P)], [m] * P, D, 1, D)
        pairs = AL.default_pairs(P, P, None)
        srch = AL._SearchLaunch(L.ALIGN_EUCLID, L.SEARCH_MEAN, rq, rd, pairs, a.n_hits, 1, 0)
        dtw = AL._Launches(L.ALIGN_DTW, L.ALIGN_EUCLID, rq, rd, pairs, False, None)
        for _ in range(a.warmup):
            srch.run(name)
            dtw.run(name)
        torch.cuda.synchronize()
        ms = {"search": [], "dtw": []}
        for _ in range(a.repeats):
            ms["search"].append(timed(lambda: srch.run(name)))
            ms["dtw"].append(timed(lambda: dtw.run(name)))
        cells = P * n * m
        rate = {}
        out.append(f"{name}: P = {P} pairs of {n} x {m}, D = {D}" + ("   (32 query rows: half of the wave's lanes idle)" if n < 64 else ""))
        for k in ("search", "dtw"):
            med = statistics.median(ms[k])
            rate[k] = cells / (med * 1e-3)
            out.append(f"  {k:6s} launch ms : " + " ".join(f"{x:.4f}" for x in ms[k]))
            out.append(f"  {k:6s} median / min / max / spread ms : {med:.4f} / {min(ms[k]):.4f} / {max(ms[k]):.4f} / "
                       f"{max(ms[k]) - min(ms[k]):.4f}   cell updates / s: {rate[k]:.4g}")
        found = int(srch.count.sum().item())
        out.append(f"  ratio search / dtw : {rate['search'] / rate['dtw']:.3f}   (hits found: {found} of {P * a.n_hits}, pairs not finite: "
                   f"{int(srch.bad[0].item())})")
        out.append("")
        del srch, dtw, rq, rd
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
