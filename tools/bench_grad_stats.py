#!/usr/bin/env python3
"""Measure the gradient noise statistics (ae_wavenet_amd/grad_analysis.py) on the headline engine, B = 8, w = 5000, and write
profiles/grad_stats.json.  Alternating windows in ONE process, medians with their spread (min .. max over the windows):

  add               GradStats.add() - one AEW_OP_GRAD_WELFORD launch over the flat gradient buffer - against the
                    reference's mu_s_incr written with torch ops as ONE expression over the same flat device buffers
                    (which already flatters it against its per-tensor loop)
  sigma_quantiles   seven quantiles of every tensor in one AEW_OP_SEG_SELECT against the per-tensor kthvalue loop on the
                    device, without the .item() calls
  step              a training step with GradStats.add() behind every backward against the plain step (recorded only)

    python tools/bench_grad_stats.py [--windows 7] [--reps 20] [--out profiles/grad_stats.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QS = [0, .1, .25, .5, .75, .9, 1]


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(xs):
    return dict(median_ms=round(statistics.median(xs), 5), min_ms=round(min(xs), 5), max_ms=round(max(xs), 5), windows=len(xs))


def alternate(a, b, windows, reps):
    """Windows of a and b in turn; ({a}, {b}, ratio of the medians, whether a's slowest window beats b's fastest)."""
    ta, tb = [], []
    a(); b()
    for _ in range(windows):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    sa, sb = summary(ta), summary(tb)
    return sa, sb, round(sb["median_ms"] / sa["median_ms"], 3), max(ta) < min(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n-win", dest="n_win", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_stats.json"))
    args = ap.parse_args()
    import ctypes as C
    import torch
    from ae_wavenet_amd import _lib as L, autoencoder_model as ae, config, grad_analysis as GA, optim
    dev = torch.device("cuda:0")
    hps = config.make_hps("vqvae-ema", n_win_batch=args.n_win, n_batch=args.batch)
    torch.manual_seed(2507)
    model = ae.AutoEncoder(hps, n_mel=39).to(dev)
    opt = optim.FusedAdam(model, lr=1e-4)
    g = model.geom
    gen = torch.Generator().manual_seed(1000)
    B = args.batch
    batch = (torch.randint(0, 256, (B, g.enc_in_len), generator=gen).float().to(dev), torch.randn(B, 39, g.mel_len, generator=gen).to(dev),
             torch.randint(0, 40, (B,), generator=gen).to(dev), torch.arange(g.embed_len).repeat(B, 1).to(dev))

    def step(gs=None):
        opt.zero_grad()
        _, _, loss = model.run(*batch)
        loss.backward()
        if gs is not None:
            gs.add()
        opt.step()

    gs = GA.GradStats(model)
    for _ in range(3):
        step(gs)
    eng = model._engine
    n = eng.ps.numel
    rec = {"numel": n, "tensors": len(gs.names), "chunks": gs.n_chunks, "batch": B, "n_win": args.n_win, "quantiles": QS}
    box = (C.c_float * 2)()
    nbytes = 90 << 20
    scratch = torch.empty(2 * nbytes, dtype=torch.uint8, device=dev)
    L.check(L.load().aew_probe_box(scratch.data_ptr(), scratch.numel(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream), box),
            "aew_probe_box")
    rec["box"] = {"mfma_bf16_tflops": round(float(box[0]), 1), "copy_90MB_TBps": round(float(box[1]), 3)}
    del scratch

    # ---- add(): the fused launch against mu_s_incr as one torch expression over the flat buffers
    grads = eng.ps.grads[:n]
    mu, s = gs.mu[:n].clone(), gs.s[:n].clone()
    state = {"mu": mu, "s": s}

    def torch_incr():
        d = grads - state["mu"]
        m2 = state["mu"] + d / 5
        state["s"] = state["s"] + d * (grads - m2)
        state["mu"] = m2

    a, b, ratio, clear = alternate(gs.add, torch_incr, args.windows, args.reps)
    a["GBps_5_words"] = round(5 * 4 * n / (a["median_ms"] * 1e-3) / 1e9, 1)
    rec["add"] = {"fused": a, "torch_one_expression": b, "speedup": ratio, "faster_by_more_than_the_spread": clear}

    # ---- sigma_quantiles(): one op against the per-tensor kthvalue loop (no .item())
    lay = gs._layout()
    ks = [GA.ranks(QS, k) for _, _, k, _ in lay]

    def torch_kth():
        out = []
        for (_, o, k, _), kk in zip(lay, ks):
            sig = (gs.s[o:o + k] / gs.count).sqrt()
            out.append(torch.stack([sig.kthvalue(j)[0] for j in kk]))
        return out

    a, b, ratio, clear = alternate(lambda: gs.sigma_quantiles(QS), torch_kth, args.windows, max(1, args.reps // 4))
    rec["sigma_quantiles"] = {"fused": a, "torch_kthvalue_loop": b, "speedup": ratio, "faster_by_more_than_the_spread": clear}

    # ---- the step with add() behind every backward against the plain step
    a, b, ratio, _ = alternate(lambda: step(gs), lambda: step(None), args.windows, max(1, args.reps // 4))
    rec["step"] = {"with_add": a, "plain": b, "plain_over_with_add": ratio}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
