#!/usr/bin/env python3
"""Measure evaluation by group (AEW_OP_EVAL_GROUPS) on the headline engine, B = 8, w = 5000, through the module surface,
and write profiles/evalgroups.txt.  ONE process; every phase runs under a time limit of its own (SIGALRM: the process
exits with 124):

  blocks    `model.evaluate()` inside a plain `model.evaluation()` block against the same call inside a
            `model.evaluation(by="voice")` block: `--rounds` alternating rounds of `--calls` calls between two device
            events, ms per call, median (min - max)
  finish    `ev.result()`, `ev.by_group()` and `ev.information()` of that model (one finalize launch each, plus the
            clones the surface makes), us per call
  finalize  the finalize launch alone on a table of `--groups` x `--codes` (251 x 4096: every voice of a large corpus
            against the full codebook), through aew_run_plan, us per launch

`--plain-only` runs the plain block alone and prints one JSON line: with `--tree` pointing at a checkout of another
commit (built, with its library in place) it times that commit's `model.evaluate()` with the same script, so that two
commits can be alternated process by process in one job.

    timeout -k 10 600 python tools/bench_eval_groups.py [--rounds 7] [--calls 100] [--out profiles/evalgroups.txt]
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def limit(seconds, what):
    def stop(sig, frame):
        sys.stderr.write(f"bench_eval_groups: phase '{what}' exceeded {seconds} s\n")
        os._exit(124)
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def spread(ts, scale=1.0, fmt="{:.3f}"):
    return (fmt + " (" + fmt + " - " + fmt + ")").format(statistics.median(ts) * scale, min(ts) * scale, max(ts) * scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n-win", dest="n_win", type=int, default=5000)
    ap.add_argument("--groups", type=int, default=251)
    ap.add_argument("--codes", type=int, default=4096)
    ap.add_argument("--tree", default=ROOT, help="checkout to import ae_wavenet_amd from (default: this one)")
    ap.add_argument("--plain-only", dest="plain_only", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalgroups.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from ae_wavenet_amd import _lib as L, autoencoder_model as ae, config
    if not torch.cuda.is_available():
        sys.exit("bench_eval_groups: needs the GPU (no time is reported without one)")
    dev = torch.device("cuda:0")
    B = args.batch
    hps = config.make_hps("vqvae-ema", n_win_batch=args.n_win, n_batch=B)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with limit(240, "build"):
        torch.manual_seed(2507)
        m = ae.AutoEncoder(hps, n_mel=39).to(dev)
        g = m.geom
        gen = torch.Generator().manual_seed(1000)
        batch = (torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(dev), torch.randn(B, 39, g.mel_len, generator=gen).to(dev),
                 torch.randint(0, hps.n_speakers, (B,), generator=gen).to(dev), torch.arange(g.embed_len).repeat(B, 1).to(dev))
        call = lambda: m.evaluate(*batch)
        with m.evaluation():
            timed(call, 20)                                         # warm-up: engine, plans, graphs
    if args.plain_only:
        with limit(240, "plain"), m.evaluation():
            ts = [timed(call, args.calls) for _ in range(args.rounds)]
        print(json.dumps(dict(label=args.label, ms_per_call=dict(median=statistics.median(ts), min=min(ts), max=max(ts)),
                              rounds=args.rounds, calls=args.calls, B=B, w=args.n_win)), flush=True)
        return
    with limit(60, "warm-up (grouped)"), m.evaluation(by="voice") as ev:
        timed(call, 20)
        ev.by_group(), ev.information()
    say(f"evaluation by group, B = {B}, w = {args.n_win}, G = {hps.n_speakers} voices, K = {hps.bn_vq_n_embed} codes, "
        f"{m._engine.Q // B} queries per window; module surface, {args.rounds} alternating rounds of {args.calls} calls in one "
        "process, HIP events; median (min - max)")
    with limit(300, "blocks"):
        t = {"plain": [], "voice": []}
        for _ in range(args.rounds):
            with m.evaluation():
                t["plain"].append(timed(call, args.calls))
            with m.evaluation(by="voice"):
                t["voice"].append(timed(call, args.calls))
        mp, mv = statistics.median(t["plain"]), statistics.median(t["voice"])
        say(f"  model.evaluate() in model.evaluation()            {spread(t['plain'])} ms")
        say(f"  model.evaluate() in model.evaluation(by='voice')  {spread(t['voice'])} ms")
        say(f"  difference of the medians {1e3 * (mv - mp):.1f} us per call ({100 * (mv / mp - 1):.2f} %): the grouped op is two dependent small "
            "launches (per window, per group) plus the device copy of the ids into in.group")
    with limit(120, "finish"), m.evaluation(by="voice") as ev:
        call()
        for name, fn in (("ev.result()", ev.result), ("ev.by_group()", ev.by_group), ("ev.information()", ev.information)):
            timed(fn, 10)
            say(f"  {name:<20s} {spread([timed(fn, 10) for _ in range(20)], 1e3, '{:.1f}')} us per call (20 windows of 10 calls)")
    with limit(120, "finalize"):
        G, K = args.groups, args.codes
        gen = torch.Generator().manual_seed(7)
        ghist = torch.randint(0, 50, (G, K), generator=gen, dtype=torch.int32).to(dev)
        rec = torch.zeros(G * 8 + 4 + K + 4 * G, dtype=torch.float64, device=dev)
        out = torch.zeros(G * 12 + 16, dtype=torch.float32, device=dev)
        op = L.Op()
        op.kind = L.OP_EVAL_GROUPS
        p = op.u.evg
        p.G, p.K, p.finalize = G, K, 1
        p.gacc, p.gtot, p.scratch = rec.data_ptr(), rec.data_ptr() + 8 * G * 8, rec.data_ptr() + 8 * (G * 8 + 4)
        p.ghist, p.gout, p.tout = ghist.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * G * 12
        lib, st = L.load(), torch.cuda.current_stream().cuda_stream
        fail = C.c_int(-1)
        fn = lambda: L.check(lib.aew_run_plan(C.byref(op), 1, C.c_void_p(st), C.byref(fail)), "finalize")
        timed(fn, 10)
        ts = [timed(fn, 10) for _ in range(20)]
        say(f"finalize launch alone, G = {G}, K = {K} ({4 * G * K / 1e6:.1f} MB table, streamed once for the column sums and once "
            f"for the row terms; three dependent kernels): {spread(ts, 1e3, '{:.1f}')} us per launch (20 windows of 10 launches)")
        say(f"  mutual information of the random table {float(out[G * 12 + 4]):.6f} bits, Miller-Madow {float(out[G * 12 + 5]):.6f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
