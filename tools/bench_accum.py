#!/usr/bin/env python3
"""Measure gradient accumulation (AEW_OP_ACCUM, `accumulate=k`) on the headline engine, B = 8, w = 5000, and write
profiles/accum.txt.  ONE process; every phase runs under a time limit of its own (SIGALRM: the process exits with 124):

  op      the three modes over the flat gradient buffer (ps.numel floats) through TrainEngine.accum_grads: `--reps`
          windows of `--burst` back-to-back launches between two device events, median (min .. max) per launch, and the
          bytes the mode has to move - FIRST 2 words per element, ADD / LAST 3 - over that time
  copy    torch's device copy over buffers that move the same bytes (n floats: 2 words per element; 1.5 n floats: 3),
          timed the same way in the same process
  step    ms per micro-batch (zero_grad, run, backward, step) of a model built with accumulate=4 against one built with
          accumulate=1, alternating windows in the same process (the accumulating model runs Adam on every 4th only)

    timeout -k 10 600 python tools/bench_accum.py [--reps 20] [--burst 10] [--windows 7] [--out profiles/accum.txt]
"""
import argparse
import contextlib
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@contextlib.contextmanager
def limit(seconds, what):
    def stop(sig, frame):
        sys.stderr.write(f"bench_accum: phase '{what}' exceeded {seconds} s\n")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8, help="micro-batches per window of the step comparison (a multiple of 4)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n-win", dest="n_win", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum.txt"))
    args = ap.parse_args()
    import torch
    from ae_wavenet_amd import _lib as L, autoencoder_model as ae, config, optim
    if not torch.cuda.is_available():
        sys.exit("bench_accum: needs the GPU (no time is reported without one)")
    dev = torch.device("cuda:0")
    hps = config.make_hps("vqvae-ema", n_win_batch=args.n_win, n_batch=args.batch)
    B = args.batch
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with limit(240, "build"):
        models = {}
        for k in (4, 1):
            torch.manual_seed(2507)
            m = ae.AutoEncoder(hps, n_mel=39, accumulate=k).to(dev)
            models[k] = (m, optim.FusedAdam(m, lr=1e-4))
        g = models[1][0].geom
        gen = torch.Generator().manual_seed(1000)
        batch = (torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(dev), torch.randn(B, 39, g.mel_len, generator=gen).to(dev),
                 torch.randint(0, 40, (B,), generator=gen).to(dev), torch.arange(g.embed_len).repeat(B, 1).to(dev))

        def micro(k):
            m, opt = models[k]
            opt.zero_grad()
            m.run(*batch)[2].backward()
            opt.step()

        for _ in range(8):                                         # warm-up: graphs captured, both groups closed
            micro(4)
            micro(1)
        torch.cuda.synchronize()
    eng = models[4][0]._engine
    n = eng.ps.numel
    say(f"gradient accumulation, B = {B}, w = {args.n_win}: ps.numel = {n} floats ({4 * n / 1e6:.1f} MB per buffer); "
        f"{args.reps} windows of {args.burst} launches, per launch: median (min .. max)")

    def report(name, words, ts):
        med = statistics.median(ts)
        say(f"  {name:<28s} {med * 1e3:8.1f} us ({min(ts) * 1e3:.1f} .. {max(ts) * 1e3:.1f})   {words * 4 * n / (med * 1e-3) / 1e12:6.3f} TB/s "
            f"({words:g} words per element)")
        return med

    with limit(120, "op"):
        op = {}
        for name, mode, words in (("accum FIRST", L.ACCUM_FIRST, 2), ("accum ADD", L.ACCUM_ADD, 3), ("accum LAST", L.ACCUM_LAST, 3)):
            fn = lambda mode=mode: eng.accum_grads(mode)
            timed(fn, args.burst)
            op[name] = report(name, words, [timed(fn, args.burst) for _ in range(args.reps)])
            eng.ps.grads[:n].normal_()                            # (LAST doubles g every launch: keep the values finite)
    with limit(120, "copy"):
        for name, elems, words in (("torch copy_, n floats", n, 2), ("torch copy_, 1.5 n floats", n + n // 2, 3)):
            src, dst = torch.randn(elems, device=dev), torch.empty(elems, device=dev)
            fn = lambda: dst.copy_(src)
            timed(fn, args.burst)
            report(name, words, [timed(fn, args.burst) for _ in range(args.reps)])
            del src, dst
    with limit(300, "step"):
        t = {4: [], 1: []}
        for _ in range(args.windows):
            for k in (4, 1):
                t[k].append(timed(lambda: micro(k), args.steps))
        m4, m1 = statistics.median(t[4]), statistics.median(t[1])
        say(f"ms per micro-batch, {args.windows} alternating windows of {args.steps} micro-batches: median (min .. max)")
        say(f"  accumulate=4 {m4:.3f} ({min(t[4]):.3f} .. {max(t[4]):.3f})   accumulate=1 {m1:.3f} ({min(t[1]):.3f} .. {max(t[1]):.3f})   "
            f"ratio {m4 / m1:.4f}")
        say(f"  (accumulate=4: one fold per micro-batch - ADD {op['accum ADD'] * 1e3:.0f} us is {100 * op['accum ADD'] / m1:.2f} % of the "
            f"accumulate=1 step - and Adam on every 4th micro-batch only)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
