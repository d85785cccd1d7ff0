#!/usr/bin/env python3
"""The training step at the benchmark shape through the module surface, fed in two ways from the same corpus:

  host    a host loop cuts the batch's windows out of a numpy corpus (what the reference's SliceDataset + collate do),
          DevicePrefetcher moves them (pinned buffer, copy stream);
  device  DeviceBatches cuts them out of the corpus in device memory (AEW_OP_WINDOW_GATHER), on the step's stream;
  device_prefetch  the same with prefetch=1: the producers run one batch ahead on the iterator's own stream.

All compute mel (DeviceMfcc) and the jitter indices (DeviceJitter) on the device.  They are timed in alternating
windows in one process (host clock around `steps` steps ending in a device synchronise, after a warm-up of both);
reported per path: every window, the median and the spread (max - min).  Against these, the time of the gather op alone
from the plan's timing interface (device events around the op's launches, aew_timing_enable).  One JSON line on stdout,
also written to --out.  Nothing is asserted: this is a record.

    python tools/bench_corpus.py --steps 100 --rounds 6 --out profiles/corpus_feed.json
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n-win", dest="n_win", type=int, default=5000)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--out", default="")
    return ap.parse_args()


def make_corpus(n_utt, slice_size, rs):
    lengths = rs.randint(slice_size + 5000, slice_size + 120000, n_utt)
    snd = rs.randint(0, 256, int(lengths.sum())).astype(np.uint8)
    samples, at = [], 0
    for i, n in enumerate(lengths):
        samples.append((i % 40, at, at + int(n)))
        at += int(n)
    return snd, samples


def host_loop(snd, starts, voices, slice_size, B, seed):
    """The reference's per-item work on the host: follow a permutation, cut the slices, stack them to floats."""
    e = 0
    while True:
        g = torch.Generator()
        g.manual_seed(seed + e)
        perm = torch.randperm(len(starts), generator=g).tolist()
        for k in range(0, len(perm) - B + 1, B):
            rows = perm[k:k + B]
            wav = torch.stack([torch.from_numpy(snd[starts[i]:starts[i] + slice_size]) for i in rows]).float()
            voice = torch.tensor([int(voices[i]) for i in rows]).long()
            yield wav, None, voice, None
        e += 1


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_corpus.py measures on the MI355X; no device found")
    device = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, corpus as CP
    from ae_wavenet_amd.jitter import DeviceJitter
    from ae_wavenet_amd.loader import DevicePrefetcher
    from ae_wavenet_amd.mfcc import DeviceMfcc
    from ae_wavenet_amd.plan import Plan
    lib = L.load()
    sys.argv = ["bench.py", "--batch", str(a.batch), "--n-win", str(a.n_win)]
    bargs = bench.parse()
    hps, model, opt = bench.make_model(bargs, device)
    eng = model._ensure_engine(a.batch)
    n = model.geom.enc_in_len
    snd, samples = make_corpus(a.utterances, n, np.random.RandomState(2507))
    corpus = CP.DeviceCorpus(snd, samples, n, hps.n_win_batch, device)
    corpus_ahead = CP.DeviceCorpus(snd, samples, n, hps.n_win_batch, device)     # (a place of its own: its stream differs)
    feeds = {
        "host": DevicePrefetcher(host_loop(snd, corpus.starts_host, corpus.voices_host, n, a.batch, 1), device, depth=2,
                                 mfcc=DeviceMfcc(device), jitter=DeviceJitter(bargs.jitter_prob, seed=11)),
        "device": CP.DeviceBatches(corpus, a.batch, mfcc=DeviceMfcc(device), jitter=DeviceJitter(bargs.jitter_prob, seed=11)),
        "device_prefetch": CP.DeviceBatches(corpus_ahead, a.batch, mfcc=DeviceMfcc(device),
                                            jitter=DeviceJitter(bargs.jitter_prob, seed=11), prefetch=1),
    }

    def step(feed):
        wav, mel, voice, jitter = next(feed)[:4]
        opt.zero_grad()
        pred, target, loss = model.run(wav, mel, voice, jitter)
        loss.backward()
        opt.step()

    def window(feed, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            step(feed)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    try:
        box = bench.box_record(lib, eng, device)
    except Exception as e:                                           # never lose the record
        box = {"error": f"{type(e).__name__}: {e}"}
    for name in feeds:
        window(feeds[name], a.warmup)
    ms = {name: [] for name in feeds}
    for r in range(a.rounds):
        names = list(feeds)
        for name in names[r % len(names):] + names[:r % len(names)]:      # the order rotates from round to round
            ms[name].append(round(window(feeds[name], a.steps), 4))

    # the gather op alone: device events around each launch (the plan's timing interface), the counter advancing
    B, pitch = a.batch, -(-n // 4) * 4
    wav = torch.empty(B, pitch, dtype=torch.float32, device=device)
    voice = torch.empty(B, dtype=torch.int64, device=device)
    index = torch.empty(B, dtype=torch.int32, device=device)
    position = torch.empty(2, dtype=torch.int64, device=device)
    plan = Plan("corpus")
    plan.add(L.OP_WINDOW_GATHER, corpus.gather_op(B, wav, voice, index, position).u.wgat, "gather")
    st = torch.cuda.current_stream(device).cuda_stream
    reps = 200
    for _ in range(20):
        corpus.note_batches(1)
        plan.run(st)
    torch.cuda.synchronize()
    lib.aew_timing_enable(1)
    for _ in range(reps):
        corpus.note_batches(1)
        plan.run(st)
    t_ms, tags, cnt = (C.c_float * reps)(), (C.c_int32 * reps)(), C.c_int(0)
    L.check(lib.aew_timing_read(t_ms, tags, reps, C.byref(cnt)), "timing_read")
    lib.aew_timing_enable(0)
    op_us = sorted(1e3 * t_ms[i] for i in range(min(cnt.value, reps)))

    def summary(v):
        return {"windows_ms": v, "median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}

    rec = {"what": "training step through the module surface, host-fed (DevicePrefetcher) vs device-fed (DeviceBatches, "
                   "prefetch 0 and 1)",
           "shape": {"batch": a.batch, "n_win": a.n_win, "slice_size": n, "corpus_samples": int(snd.size),
                     "slices": len(corpus)},
           "method": f"alternating windows of {a.steps} steps, {a.rounds} per path, warm-up {a.warmup} steps per path; "
                     "host clock around steps that end in a device synchronise",
           "host_fed": summary(ms["host"]), "device_fed": summary(ms["device"]),
           "device_fed_prefetch": summary(ms["device_prefetch"]),
           "gather_op_us": {"launches": len(op_us), "median": round(statistics.median(op_us), 2),
                            "min": round(op_us[0], 2), "max": round(op_us[-1], 2),
                            "note": "both launches of the op (gather + counter advance), device events around them"},
           "bytes": {"in": a.batch * n * corpus.snd_bytes, "out": a.batch * n * 4},
           "box": box}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
