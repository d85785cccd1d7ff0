#!/usr/bin/env python3
"""AEW_OP_CODE_SEGMENT at the sizes its callers have, in FRAMES PER SECOND:

  corpus_4096   4096 utterances x 500 frames at K = 4096, d = 64, scaled_l2   (ten seconds at 50 Hz, the flagship codebook)
  corpus_512    the same at K = 512
  lone          one utterance of 1000 frames at K = 4096                       (the latency of a lone utterance)

Method.  The utterances go through the op in chunks of at most `--chunk-frames` rows (the local costs of a chunk take
rows * K * 4 bytes), every chunk with its own op record, built once.  Per case `--warmup` passes over all chunks, then
`--repeats` (>= 7) timed passes, each between two device events on torch's current stream; median, minimum, maximum and
spread are reported and frames/s at the median.  The op is two kernels in one launch.  They are told apart with a second
set of records whose utterances are all EMPTY: k_seg_cost does the same work on the same rows, k_seg_scan returns at
once - that pass is reported as `cost_ms`, and `scan_ms` is the whole pass minus it (both from device events, the
second a difference).

Two figures stand beside each case, named for what they are:

  valu_ceiling   frames/s of k_seg_cost if nothing but the 2 * K * d lane operations of a frame's distances (one subtract
                 and one fused multiply-add per channel and entry) were issued: the guide's 64 fp32 FLOP per clock per
                 SIMD counts a packed fused multiply-add on 16 lanes, un-packed that is 16 lane operations per clock per
                 SIMD; times 4 SIMDs per CU, the CUs and the clock the box reports.  Derived, not measured; the
                 square root, the division and the store come on top, so no kernel reaches it.
  torch_cpu      the same rule taken by torch on 16 CPU threads on the first `--cpu-utterances` utterances (all their
                 frames against the codebook by broadcasting, the recurrence one frame of all utterances at a time).

With --corpus the tool also times model.segment_corpus() next to model.encode_corpus() on one synthetic corpus (the
default vqvae-ema model, random weights).  One JSON line on stdout, also written to --out with a readable table in front
of it.  Nothing is asserted about speed: this is a record.

    timeout -k 10 900 python tools/bench_segment.py --corpus --out profiles/segment.txt
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--utterances", type=int, default=4096)
    ap.add_argument("--chunk-frames", dest="chunk", type=int, default=1 << 19)
    ap.add_argument("--cpu-utterances", dest="cpu_utts", type=int, default=8)
    ap.add_argument("--penalty", type=float, default=0.05)
    ap.add_argument("--cases", default="corpus_4096,corpus_512,lone")
    ap.add_argument("--corpus", action="store_true")
    ap.add_argument("--out", default="")
    return ap.parse_args()


def cpu_segment(z, emb, lam):
    """z (P, T, d), emb (K, d) fp32 CPU tensors -> codes (P, T): the rule (scaled_l2) with torch, all utterances at once."""
    P, T, d = z.shape
    K = emb.shape[0]
    en = emb.square().sum(1).sqrt()
    c = torch.empty(P, T, K)
    for t in range(T):
        diff = z[:, t, None, :] - emb[None]
        c[:, t] = diff.square().sum(2).sqrt() / (z[:, t].square().sum(1).sqrt()[:, None] + en[None])
    stay = torch.zeros(P, T, K, dtype=torch.bool)
    A = torch.zeros(P, T, dtype=torch.int64)
    r = c[:, 0].clone()
    for t in range(1, T):
        m, a = r.min(1)
        A[:, t - 1] = a
        p = r - m[:, None]
        stay[:, t] = p < lam
        r = c[:, t] + torch.where(stay[:, t], p, torch.full_like(p, lam))
    k = r.argmin(1)
    codes = torch.zeros(P, T, dtype=torch.int64)
    rows = torch.arange(P)
    for t in range(T - 1, 0, -1):
        codes[:, t] = k
        k = torch.where(stay[rows, t, k], k, A[:, t - 1])
    codes[:, 0] = k
    return codes


def device_clock(props):
    """(Hz, where the figure comes from): the engine clock the box reports, else the part's peak engine clock - the one
    behind its 157.3 TFLOP/s vector fp32 figure (256 CUs x 4 SIMDs x 64 FLOP x 2.4 GHz)."""
    if hasattr(props, "clock_rate"):
        return props.clock_rate * 1e3, "torch device properties (clock_rate)"
    return 2.4e9, "the part's peak engine clock, 2.4 GHz (this torch reports none in the device properties)"


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def stats(ms):
    return {"launch_ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_segment.py measures on the MI355X; no device found")
    if a.repeats < 7:
        sys.exit("at least 7 repeats")
    dev = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, codes as CD
    L.load()
    torch.set_num_threads(16)
    props = torch.cuda.get_device_properties(0)
    clock_hz, clock_from = device_clock(props)
    lane_ops = 16 * 4 * props.multi_processor_count * clock_hz
    rec = {"what": "AEW_OP_CODE_SEGMENT: frames per second", "cases": {},
           "method": f"{a.warmup} warm-up passes, {a.repeats} timed passes between device events, per case; frames/s at the "
                     "median; cost_ms: the same pass with every utterance empty (k_seg_cost alone), scan_ms: the difference",
           "valu_ceiling": {"derivation": "16 lane operations per clock per SIMD (64 fp32 FLOP per clock per SIMD is a packed "
                                          "FMA on 16 lanes) x 4 SIMDs x CUs x clock; 2 * K * d lane operations per frame",
                            "cus": props.multi_processor_count, "clock_hz": clock_hz, "clock_from": clock_from,
                            "lane_ops_per_s": lane_ops},
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
                   "torch": torch.__version__, "hip": getattr(torch.version, "hip", None), "cpu_threads": torch.get_num_threads()}}
    cases = {"corpus_4096": (a.utterances, 500, 4096), "corpus_512": (a.utterances, 500, 512), "lone": (1, 1000, 4096)}
    d = 64
    for name in a.cases.split(","):
        U, T, K = cases[name]
        gen = torch.Generator().manual_seed(len(name))
        emb_h = torch.randn(K, d, generator=gen)
        # frames that dwell: a random walk between entries, so that the penalty has segments to find
        z_h = emb_h[torch.randint(0, K, (U, T // 10 + 1), generator=gen)].repeat_interleave(10, 1)[:, :T] \
            + 0.7 * torch.randn(U, T, d, generator=gen)
        emb, z = emb_h.to(dev), z_h.to(dev)
        per = max(1, a.chunk // T)
        launches, empties, keep = [], [], []
        for lo in range(0, U, per):
            hi = min(U, lo + per)
            frames = z[lo:hi].reshape(-1, d)
            for lam, into in ((a.penalty, launches), (None, empties)):
                n = frames.shape[0]
                plan = CD.segment_plan([T] * (hi - lo) if lam is not None else [0] * (hi - lo), K)
                plan.table["lam"] = 0.0 if lam is None else lam
                host = torch.empty(plan.table.nbytes, dtype=torch.uint8, pin_memory=True)
                host.numpy()[:] = plan.table.view(np.uint8).reshape(-1)
                table = host.to(dev)
                out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
                       torch.empty(hi - lo, dtype=torch.float32, device=dev), torch.empty(hi - lo, dtype=torch.int32, device=dev),
                       torch.zeros(1, dtype=torch.int32, device=dev))
                cs = L.CodeSegment()
                cs.frames, cs.n_elems, cs.emb = frames.data_ptr(), frames.numel(), emb.data_ptr()
                cs.K, cs.d, cs.d_pitch, cs.metric = K, d, d, 0
                cs.table, cs.table_host, cs.U = table.data_ptr(), host.data_ptr(), hi - lo
                cs.codes, cs.dist, cs.n_out = out[0].data_ptr(), out[1].data_ptr(), n
                cs.cost, cs.n_seg, cs.n_bad = out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr()
                into.append(cs)
                keep.append((host, table, out, frames))
        ws_bytes = CD.segment_ws_bytes(min(per, U) * T, K)
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)        # one workspace, the chunks follow each other
        for cs in launches + empties:
            cs.ws, cs.ws_bytes = ws.data_ptr(), ws_bytes

        def run(recs):
            for cs in recs:
                CD._run(L.OP_CODE_SEGMENT, cs, name, dev)

        whole = timed(lambda: run(launches), a.warmup, a.repeats)
        cost = timed(lambda: run(empties), a.warmup, a.repeats)
        run(launches)
        torch.cuda.synchronize()
        n_frames = U * T
        med, cmed = statistics.median(whole), statistics.median(cost)
        ceiling = lane_ops / (2 * K * d)
        cp = max(1, min(a.cpu_utts, U))
        cpu_segment(z_h[:1, :50], emb_h, a.penalty)
        t0 = time.perf_counter()
        ref = cpu_segment(z_h[:cp], emb_h, a.penalty)
        cpu_s = time.perf_counter() - t0
        got = keep[0][2][0][:cp * T].view(cp, T).cpu()
        n_seg = torch.cat([k[2][3] for k in keep[::2]]).float()
        case = {"utterances": U, "frames_each": T, "K": K, "d": d, "penalty": a.penalty, "chunks": len(launches),
                "workspace_bytes": ws_bytes, "whole": stats(whole), "frames_per_s": round(n_frames / (med * 1e-3)),
                "cost_ms": stats(cost), "scan_ms_by_difference": round(med - cmed, 4),
                "cost_frames_per_s": round(n_frames / (cmed * 1e-3)),
                "valu_ceiling_frames_per_s": round(ceiling),
                "cost_fraction_of_valu_ceiling": round(n_frames / (cmed * 1e-3) / ceiling, 4),
                "mean_segments": round(float(n_seg.mean()), 2),
                "torch_cpu": {"utterances": cp, "threads": torch.get_num_threads(), "seconds": round(cpu_s, 3),
                              "frames_per_s": round(cp * T / cpu_s),
                              "codes_equal_to_device": round(float((ref == got).float().mean()), 4)}}
        rec["cases"][name] = case
        del launches, empties, keep, ws, z, emb
        torch.cuda.empty_cache()
    if a.corpus:
        rec["corpus"] = corpus_timing(dev)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for name, c in rec["cases"].items():
                fh.write(f"{name:12s} U={c['utterances']:5d} T={c['frames_each']:4d} K={c['K']:4d}  whole {c['whole']['median_ms']:9.3f} ms"
                         f"  {c['frames_per_s']:>12,d} frames/s | k_seg_cost {c['cost_ms']['median_ms']:9.3f} ms"
                         f" ({100 * c['cost_fraction_of_valu_ceiling']:.1f} % of the VALU ceiling {c['valu_ceiling_frames_per_s']:,d} frames/s)"
                         f" | k_seg_scan {c['scan_ms_by_difference']:9.3f} ms | torch cpu {c['torch_cpu']['frames_per_s']:,d} frames/s\n")
            if "corpus" in rec:
                c = rec["corpus"]
                fh.write(f"corpus: {c['utterances']} utterances, {c['codes']} codes: encode_corpus {c['encode_corpus_s']:.3f} s, "
                         f"segment_corpus {c['segment_corpus_s']:.3f} s\n")
            fh.write(line + "\n")


def corpus_timing(dev, U=64, seconds=2.0):
    """Wall clock of encode_corpus() and segment_corpus() over one synthetic corpus (second call of each, synchronised)."""
    from ae_wavenet_amd import autoencoder_model as ae, config, corpus as CP
    hps = config.make_hps("vqvae-ema")
    torch.manual_seed(0)
    m = ae.AutoEncoder(hps, n_mel=3 * hps.n_mfcc).to(dev)
    n = int(seconds * hps.sample_rate)
    rs = np.random.RandomState(0)
    snd = rs.randint(0, 256, U * n).astype(np.uint8)
    samples = [CP.SpokenSample(voice_index=u % 5, wav_b=u * n, wav_e=(u + 1) * n, file_path=f"u{u}") for u in range(U)]
    corpus = CP.DeviceCorpus.from_arrays(snd, samples, 1000, 500, dev)
    out = {"utterances": U, "seconds_each": seconds, "K": int(hps.bn_vq_n_embed)}
    for key, fn in (("encode_corpus_s", lambda: m.encode_corpus(corpus, batch=8, return_dist=True)),
                    ("segment_corpus_s", lambda: m.segment_corpus(corpus, 0.05, batch=8, return_dist=True))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        uc = fn()
        torch.cuda.synchronize()
        out[key] = round(time.perf_counter() - t0, 4)
        out["codes"] = int(uc.codes.numel())
    return out


if __name__ == "__main__":
    main()
