#!/usr/bin/env python3
"""Tokenising whole utterances at the headline geometry (vqvae-ema, B = 8, n_win 5000), from the same whole-utterance
mels on the device to the same codes, in two ways:

  loop    the only way without model.encode_utterances(): a host loop cuts every window out of its utterance's mel,
          zero-pads it, stacks B of them, calls model.encode() and cuts the codes whose receptive field lies inside
          real frames out of the result (windows of all utterances packed B per call, the best such a loop can do);
  device  model.encode_utterances(): one table upload per call, AEW_OP_MEL_TILE / AEW_OP_CODE_STITCH around the same
          encode plan per batch.

Both give the same codes, bit for bit (checked before anything is timed).  They are timed in alternating windows in one
process (host clock around `calls` calls ending in a device synchronise, after a warm-up of both); per path: every
window, the median and the spread (max - min), codes/s and utterances/s at the median.  `wavs` is
model.encode_wavs() over the same corpus - the whole-utterance MFCC included -, timed the same way, for the record.  One
JSON line on stdout, also written to --out.  Nothing is asserted about speed: this is a record.

    timeout -k 10 600 python tools/bench_tokenise.py --rounds 7 --calls 5 --out profiles/tokenise.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="corpus passes per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n-win", dest="n_win", type=int, default=5000)
    ap.add_argument("--utterances", type=int, default=48)
    ap.add_argument("--seconds", default="2,12", help="utterance lengths, uniform between these (16 kHz)")
    ap.add_argument("--out", default="")
    return ap.parse_args()


def loop_encode(model, mels, B, E, s, rf, mel_len):
    """What a caller of model.encode() has to do for whole utterances: returns the flat codes."""
    dev = mels[0].device
    out, rows, keep = [], [], []

    def flush():
        x = torch.zeros(B, mels[0].shape[0], mel_len, device=dev)
        for b, w in enumerate(rows):
            x[b, :, :w.shape[1]] = w
        codes = model.encode(x)
        out.extend(codes[b, :k] for b, k in enumerate(keep))
        rows.clear()
        keep.clear()

    for m in mels:
        F = m.shape[1]
        N = 0 if F < rf else (F - rf) // s + 1
        for w in range(-(-N // E)):
            rows.append(m[:, w * s * E:w * s * E + mel_len])
            keep.append(min(E, N - w * E))
            if len(rows) == B:
                flush()
    if rows:
        flush()
    return torch.cat(out)


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_tokenise.py measures on the MI355X; no device found")
    device = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, geometry as G
    from ae_wavenet_amd.mfcc import DeviceMfcc
    lib = L.load()
    sys.argv = ["bench.py", "--batch", str(a.batch), "--n-win", str(a.n_win)]
    bargs = bench.parse()
    hps, model, opt = bench.make_model(bargs, device)
    eng = model._ensure_engine(a.batch)
    E, s, rf, mel_len = G.utterance_geometry(eng.geom)
    lo, hi = (float(x) for x in a.seconds.split(","))
    rs = np.random.RandomState(2611)
    lengths = rs.randint(int(lo * hps.sample_rate), int(hi * hps.sample_rate), a.utterances)
    wavs = [torch.from_numpy(rs.randint(0, 256, int(n)).astype(np.float32)).to(device) for n in lengths]
    mf = DeviceMfcc(device, hps.sample_rate, hps.mfcc_win_sz, hps.mfcc_hop_sz, hps.n_mels, hps.n_mfcc)
    mels = [mf(w[None])[0] for w in wavs]
    frames = [int(m.shape[1]) for m in mels]

    paths = {"loop": lambda: loop_encode(model, mels, a.batch, E, s, rf, mel_len),
             "device": lambda: model.encode_utterances(mels, batch=a.batch).codes,
             "wavs": lambda: model.encode_wavs(wavs, batch=a.batch).codes}
    ref = paths["loop"]()
    n_codes = int(ref.numel())
    same = {name: bool(torch.equal(paths[name](), ref)) for name in ("device", "wavs")}

    def window(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    try:
        box = bench.box_record(lib, eng, device)
    except Exception as e:                                           # never lose the record
        box = {"error": f"{type(e).__name__}: {e}"}
    for name in paths:
        window(paths[name], a.warmup)
    ms = {name: [] for name in paths}
    for r in range(a.rounds):
        names = list(paths)
        for name in names[r % len(names):] + names[:r % len(names)]:      # the order rotates from round to round
            ms[name].append(round(window(paths[name], a.calls), 4))

    # the two ops and the encode plan alone, one batch: device events around each launch (the plan's timing interface)
    from ae_wavenet_amd import codes as CD
    from ae_wavenet_amd.plan import Plan
    tp = CD.tile_plan(frames, E, s, rf, a.batch)
    bases = np.concatenate([[0], np.cumsum([m.numel() for m in mels])])[:-1]
    tbl = tp.table(bases)
    host = torch.empty(tbl.nbytes, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = tbl.view(np.uint8).reshape(-1)
    dev_tbl = host.to(device)
    flat = torch.cat([m.reshape(-1) for m in mels])
    codes = torch.empty(n_codes, dtype=torch.int64, device=device)
    dist = torch.empty(n_codes, dtype=torch.float32, device=device)
    bp = eng.utterance_batch_plan(flat, dev_tbl, host, 0, codes, dist)
    st = torch.cuda.current_stream(device).cuda_stream
    reps, op_us = 200, {}
    for name, lo_i, hi_i in (("mel_tile", 0, 1), ("encode_plan", 1, len(bp.ops) - 1), ("code_stitch", len(bp.ops) - 1, len(bp.ops))):
        sub = Plan(name)
        sub.ops, sub.labels = bp.ops[lo_i:hi_i], bp.labels[lo_i:hi_i]
        for _ in range(20):
            sub.run(st)
        torch.cuda.synchronize()
        lib.aew_timing_enable(2)
        n_ev = reps * len(sub.ops)
        for _ in range(reps):
            sub.run(st)
        t_ms, tags, cnt = (C.c_float * n_ev)(), (C.c_int32 * n_ev)(), C.c_int(0)
        L.check(lib.aew_timing_read(t_ms, tags, n_ev, C.byref(cnt)), "timing_read")
        lib.aew_timing_enable(0)
        per = sorted(1e3 * sum(t_ms[r * len(sub.ops) + i] for i in range(len(sub.ops))) for r in range(reps))
        op_us[name] = {"launches": len(sub.ops), "median": round(statistics.median(per), 2), "min": round(per[0], 2),
                       "max": round(per[-1], 2)}
    op_us["note"] = ("device events around each launch, summed over the launches of the part; encode_plan: the ops of "
                     "_cond_plan_a one by one, eager")
    op_us["bytes"] = {"mel_tile_out": a.batch * int(mels[0].shape[0]) * mel_len * 4, "code_stitch_out": a.batch * E * 12}

    def summary(v):
        med = statistics.median(v)
        return {"windows_ms": v, "median_ms": round(med, 4), "spread_ms": round(max(v) - min(v), 4),
                "codes_per_s": round(n_codes / (med * 1e-3)), "utterances_per_s": round(a.utterances / (med * 1e-3), 1)}

    n_windows = sum(-(-(0 if F < rf else (F - rf) // s + 1) // E) for F in frames)
    rec = {"what": "whole utterances -> codes from device-resident mels: host loop over model.encode() vs "
                   "model.encode_utterances(); model.encode_wavs() (MFCC included) for the record",
           "shape": {"batch": a.batch, "n_win": a.n_win, "embed_len": E, "mel_len": mel_len, "stride": s, "rf": rf,
                     "utterances": a.utterances, "frames": int(sum(frames)), "codes": n_codes, "windows": n_windows,
                     "batches": -(-n_windows // a.batch), "audio_s": round(float(lengths.sum()) / hps.sample_rate, 1)},
           "method": f"alternating windows of {a.calls} passes over the corpus, {a.rounds} per path, warm-up {a.warmup} "
                     "passes per path; host clock around passes that end in a device synchronise",
           "same_codes_as_loop": same,
           "loop": summary(ms["loop"]), "device": summary(ms["device"]), "wavs": summary(ms["wavs"]),
           "loop_ms_over_device_ms": round(statistics.median(ms["loop"]) / statistics.median(ms["device"]), 3),
           "one_batch_us": op_us, "box": box}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
