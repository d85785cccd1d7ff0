#!/usr/bin/env python3
"""Time of the Adam launch with parameter groups at the benchmark's size (arch.vqvae-ema: 23.6 M parameters, the flat
layout of its named_parameters()), through the C ABI:

  (a) plain launch                       (b) tracked launch (update / weight ratios)
  (c) grouped, nothing frozen, no decay  (d) grouped with decay on every tensor
  (e) grouped, encoder.* + bottleneck.* frozen
  (f) grouped, everything but the speaker embedding frozen

Device events around --launches launches after a warm-up, the variants alternated inside one process, --reps repetitions;
median and spread (min .. max) per variant, and the bytes each variant touches (p, g, m, v: 16 bytes per trainable element
read, 12 written).  Appends its lines to --out."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ae_wavenet_amd import _lib as L, autoencoder_model as ae, config
    from ae_wavenet_amd.plan import Plan
    dev = "cuda:0"
    hps = config.make_hps("vqvae-ema")
    model = ae.AutoEncoder(hps)
    names, lens = [], []
    for k, p in model.named_parameters():
        names.append(k)
        lens.append(p.numel())
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 3) // 4 * 4
    total = o
    P = len(names)
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(total, generator=gen).to(dev)
    g = (torch.randn(total, generator=gen) * 0.01).to(dev)
    m, v = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
    chunks_host, first = L.uw_chunks(offs, lens)
    nch = first[-1]
    chunks = torch.frombuffer(bytearray(bytes(chunks_host))[:16 * nch], dtype=torch.int64).to(dev)
    part = torch.zeros(2 * nch, dtype=torch.float64, device=dev)
    tr = L.UwTrack()
    tr.chunks, tr.chunks_host, tr.n_chunks, tr.part, tr.base, tr.zero = chunks.data_ptr(), C.addressof(chunks_host), nch, part.data_ptr(), 0, 1

    def table(records):
        t = torch.frombuffer(bytearray(L.adam_tensor_records(records, P)), dtype=torch.int32).to(dev)
        gr = L.AdamGroups()
        gr.chunks, gr.chunks_host, gr.n_chunks = chunks.data_ptr(), C.addressof(chunks_host), nch
        gr.tensors, gr.n_tensors, gr.base = t.data_ptr(), P, 0
        return t, gr

    head = lambda k: k.startswith(("encoder.", "bottleneck."))
    tables = {
        "c": table([(1e-4, 0.0, False)] * P),
        "d": table([(1e-4, 1e-2, False)] * P),
        "e": table([(1e-4, 0.0, head(k)) for k in names]),
        "f": table([(1e-4, 0.0, "speaker_embedding" not in k) for k in names]),
    }
    trainable = {"a": total, "b": total, "c": total, "d": total,
                 "e": sum((n + 3) // 4 * 4 for k, n in zip(names, lens) if not head(k)),
                 "f": sum((n + 3) // 4 * 4 for k, n in zip(names, lens) if "speaker_embedding" in k)}
    plans = {}
    for key in "abcdef":
        a = L.Adam()
        a.p, a.g, a.m, a.v, a.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), total
        a.lr, a.beta1, a.beta2, a.eps, a.grad_scale, a.bc1, a.bc2 = 1e-4, 0.9, 0.999, 1e-8, 1.0, 0.1, 0.001
        if key == "b":
            a.track = C.addressof(tr)
        pl = Plan("adam " + key)
        if key in tables:
            ag = L.AdamGrouped()
            ag.adam, ag.groups = a, C.addressof(tables[key][1])
            pl.add(L.OP_ADAM_GROUPS, ag, "adam (groups)")
        else:
            pl.add(L.OP_ADAM, a, "adam")
        plans[key] = pl
    st = torch.cuda.current_stream().cuda_stream
    times = {k: [] for k in plans}
    for k in plans:
        for _ in range(args.warmup):
            plans[k].run(st)
    torch.cuda.synchronize()
    for rep in range(args.reps):
        for k in plans:                                             # alternated: every repetition runs every variant
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                plans[k].run(st)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    what = {"a": "plain", "b": "tracked", "c": "grouped, nothing frozen, no decay", "d": "grouped, decay on every tensor",
            "e": "grouped, encoder.* + bottleneck.* frozen", "f": "grouped, all but the speaker embedding frozen"}
    lines = [f"Adam launch, {total} elements in {P} tensors, {nch} chunks; {args.launches} launches per measurement, "
             f"{args.reps} repetitions, variants alternated; us per launch: median (min .. max)"]
    for k in plans:
        t = times[k]
        med = statistics.median(t)
        mb = trainable[k] * 28 / 1e6
        lines.append(f"({k}) {what[k]:48s} {med:8.2f} ({min(t):8.2f} .. {max(t):8.2f})  {mb:8.1f} MB moved, "
                     f"{mb / 1e6 / (med * 1e-6):6.2f} TB/s")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
