#!/usr/bin/env python3
"""ABX over an item set at the sizes a unit-discovery evaluation has: N = 2048 and N = 4096 items of 30 - 80 frames at
D = 64, 40 categories x 8 speakers, modes within / across / any.  In ONE process, alternating within every round:

  op      AEW_OP_ABX_COUNT alone over a distance matrix computed beforehand (tables uploaded once, one record): a BATCH
          of 50 launches back to back between the two events, the time divided by 50 - the enqueue (the launcher's host
          checks included) runs ahead of the device, so this is the op's time per launch in a stream that is kept
          busy, not a kernel time from a trace
  task    align.abx_task from the features: all N (N - 1) / 2 DTWs, the mirror writes, the tables, the op, the aggregation
  dtw     align.distance_matrix alone - its share of the task is the "share of the task spent in DTW"
  torch   the same counts as a blocked broadcast compare in torch on the same GPU (per speaker and A group one
          (|X|, |A|, items of the speaker) comparison, summed over A, then summed into B's groups)
  numpy   that formulation in numpy on 16 CPU threads, at the smaller size only

Each is timed between device events (numpy: a host clock) `--repeats` (>= 7) times after `--warmup` runs; median, minimum,
maximum and spread are recorded, rates at the median.  The counts of torch and numpy are compared with the op's, word for
word.  The op's rate is also set against two ceilings: the vector ALU (the inner loop is 4 vector instructions per
(a, b) pair and lane - two compares, a select, an add with carry - and a wave64 instruction issues over 2 clocks on a
SIMD-32) and the one read of the N x N matrix.  Nothing is asserted about speed: this is a record.

    timeout -k 10 1100 python tools/bench_abx.py --out profiles/abx.txt
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import numpy as np
import torch

N_CAT, N_SPK, D, CLOCK_HZ, VALU_PER_PAIR, OP_BATCH = 40, 8, 64, 2.4e9, 4, 50


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="2048,4096")
    ap.add_argument("--numpy-size", dest="numpy_size", type=int, default=2048)
    ap.add_argument("--out", default="")
    return ap.parse_args()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"ms": [round(x, 4) for x in ms], "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def blocked_counts(Ds, tb, xp):
    """(n, wrong2) as (N, G) int64 from the SORTED matrix Ds = D[perm][:, perm]; xp = torch or numpy.  Per speaker s and
    A group (cX, s): X = A's own items (within) or the items of cX under the other speakers (across); one
    (|X|, |A|, items of s) comparison, summed over A, then over the columns of every B group of s."""
    N, G, g = tb.N, tb.G, tb.groups
    is_t = xp is torch
    n = torch.zeros(N, G, dtype=torch.int64, device=Ds.device) if is_t else np.zeros((N, G), np.int64)
    w = torch.zeros_like(n) if is_t else np.zeros_like(n)
    jobs = []
    for ga in range(G):
        alo, ahi, cx, s = (int(v) for v in g[ga])
        mine = np.flatnonzero(g["spk"] == s)
        slo, shi = int(g["lo"][mine[0]]), int(g["hi"][mine[-1]])                 # the items of speaker s: one sorted range
        if tb.op_mode == 0:
            xs = np.arange(alo, ahi)
        else:
            xs = np.concatenate([np.arange(int(g["lo"][k]), int(g["hi"][k])) for k in range(G)
                                 if g["cat"][k] == cx and g["spk"][k] != s] or [np.zeros(0, np.int64)])
        if xs.size:
            jobs.append((ga, alo, ahi, cx, slo, shi, mine, xs))

    def one(job):
        ga, alo, ahi, cx, slo, shi, mine, xs = job
        xi = torch.from_numpy(xs).to(Ds.device) if is_t else xs
        da, db = Ds[xi, alo:ahi][:, :, None], Ds[xi, slo:shi][:, None, :]
        gt, lt = da > db, da < db
        per_b = (2 * gt + ~(gt | lt)).sum(1)                                     # (|X|, items of s)
        n_a = ahi - alo
        if tb.op_mode == 0:                                                      # x is one of the a's: take its pair off again
            dx = Ds[xi, xi][:, None]
            g2, l2 = dx > db[:, 0, :], dx < db[:, 0, :]
            per_b = per_b - (2 * g2 + ~(g2 | l2))
            n_a -= 1
        if n_a < 1:
            return
        for k in mine:
            if g["cat"][k] == cx:
                continue
            lo, hi = int(g["lo"][k]) - slo, int(g["hi"][k]) - slo
            w[xi, int(k)] = per_b[:, lo:hi].sum(1)
            n[xi, int(k)] = n_a * (hi - lo)

    if is_t:
        for job in jobs:
            one(job)
    else:
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(one, jobs))
    return n, w


def main():
    a = parse()
    if not torch.cuda.is_available():
        sys.exit("bench_abx.py measures on the MI355X; no device found")
    if a.repeats < 7:
        sys.exit("at least 7 repeats")
    dev = torch.device("cuda", 0)
    from ae_wavenet_amd import _lib as L, align as AL
    L.load()
    torch.set_num_threads(16)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    lane_ops = cus * 4 * 32 * CLOCK_HZ
    rec = {"what": "AEW_OP_ABX_COUNT and align.abx_task", "cases": {},
           "box": {"device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": cus, "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None), "cpu_threads": 16},
           "method": f"{a.warmup} warm-up runs, then {a.repeats} rounds of op, task, dtw, torch in turn, each between device "
                     "events; op: 50 launches back to back between the events, per launch; rates at the median",
           "valu_ceiling": {"derivation": "a wave64 vector instruction issues over 2 clocks on a SIMD-32: 32 lane operations "
                            "per clock per SIMD x 4 SIMDs x CUs x clock; 4 vector instructions per (a, b) pair and lane in "
                            "the inner loop (v_cmp_gt, v_cmp_nlt, v_cndmask, v_addc)", "cus": cus, "clock_hz": CLOCK_HZ,
                            "clock_from": "the part's peak engine clock, 2.4 GHz", "lane_ops_per_s": lane_ops,
                            "pairs_per_s": lane_ops / VALU_PER_PAIR}}
    out = []
    for N in (int(x) for x in a.sizes.split(",")):
        rs = np.random.RandomState(N)
        lens = rs.randint(30, 81, N)
        flat = torch.from_numpy(rs.randn(int(lens.sum()), D).astype(np.float32)).to(dev).reshape(-1)
        base = np.concatenate([[0], np.cumsum(lens * D)[:-1]])
        items = AL.Ragged(flat, base.tolist(), lens.tolist(), D, 1, D)
        cat, spk = rs.randint(0, N_CAT, N).tolist(), rs.randint(0, N_SPK, N).tolist()
        cells = int(sum(int(lens[i]) * int(lens[i + 1:].sum()) for i in range(N)))
        dist = AL.distance_matrix(items)
        torch.cuda.synchronize()
        for mode in ("within", "across", "any"):
            tb = AL.abx_tables(cat, spk, mode)
            partner = np.ascontiguousarray(tb.partner)
            d_tabs = [AL._upload(t, dev) for t in (tb.perm, tb.groups, partner)]
            n = torch.empty(N, tb.G, dtype=torch.int32, device=dev)
            w = torch.empty(N, tb.G, dtype=torch.int32, device=dev)
            r = L.AbxCount()
            r.mode, r.N, r.G, r.C, r.S, r.ld = tb.op_mode, N, tb.G, tb.C, tb.S, N
            r.dist, r.n, r.wrong2 = dist.data_ptr(), n.data_ptr(), w.data_ptr()
            r.perm, r.groups, r.partner = (t.data_ptr() for t in d_tabs)
            r.perm_host, r.groups_host, r.partner_host = tb.perm.ctypes.data, tb.groups.ctypes.data, partner.ctypes.data
            op = L.Op()
            op.kind, op.u.abx = L.OP_ABX_COUNT, r
            st = torch.cuda.current_stream(dev).cuda_stream

            def run_op():
                L.check(L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(st), None), "abx count")

            perm = torch.from_numpy(tb.perm.astype(np.int64)).to(dev)
            Ds = dist[perm][:, perm].contiguous()
            def run_ops():
                for _ in range(OP_BATCH):
                    run_op()

            runs = {"op": run_ops, "task": lambda: AL.abx_task(items, cat, spk, mode=mode),
                    "dtw": lambda: AL.distance_matrix(items), "torch": lambda: blocked_counts(Ds, tb, torch)}
            for _ in range(a.warmup):
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(a.repeats):
                for k, fn in runs.items():
                    ms[k].append(timed(fn) / (OP_BATCH if k == "op" else 1))
            tn, tw = blocked_counts(Ds, tb, torch)
            same_torch = bool(torch.equal(tn, n.to(torch.int64))) and bool(torch.equal(tw, w.to(torch.int64)))
            res = AL.abx_task(items, cat, spk, mode=mode)
            triples = int(res.n_triples)
            case = {k: stats(v) for k, v in ms.items()}
            med = {k: case[k]["median_ms"] * 1e-3 for k in runs}
            pairs_s, bytes_s = triples / med["op"], 4.0 * N * N / med["op"]
            case.update({"N": N, "G": tb.G, "triples": triples, "dtw_cells": cells, "error": float(res.error),
                         "pooled": float(res.pooled), "op_pairs_per_s": pairs_s,
                         "op_fraction_of_valu_ceiling": pairs_s / (lane_ops / VALU_PER_PAIR),
                         "op_matrix_bytes_per_s": bytes_s, "dtw_share_of_task": med["dtw"] / med["task"],
                         "torch_over_op": med["torch"] / med["op"], "torch_counts_equal": same_torch})
            line = (f"N={N:5d} {mode:6s} G={tb.G:4d} triples={triples:12,d} | op, per launch of 50 {case['op']['median_ms']:9.4f} ms "
                    f"({pairs_s:.3g} pairs/s = {100 * case['op_fraction_of_valu_ceiling']:.2f} % of the VALU ceiling "
                    f"{lane_ops / VALU_PER_PAIR:.3g}; matrix read at {bytes_s / 1e9:.1f} GB/s) | task "
                    f"{case['task']['median_ms']:9.3f} ms, dtw {case['dtw']['median_ms']:9.3f} ms = "
                    f"{100 * case['dtw_share_of_task']:.1f} % of it | torch {case['torch']['median_ms']:9.3f} ms = "
                    f"{case['torch_over_op']:.0f} x the op, counts equal: {same_torch}")
            if N == a.numpy_size:
                Dh = Ds.cpu().numpy()
                t0 = time.perf_counter()
                hn, hw = blocked_counts(Dh, tb, np)
                sec = time.perf_counter() - t0
                same_np = bool(np.array_equal(hn, n.cpu().numpy())) and bool(np.array_equal(hw, w.cpu().numpy()))
                case["numpy_16_threads"] = {"seconds": round(sec, 4), "over_op": sec / med["op"], "counts_equal": same_np}
                line += f" | numpy, 16 threads {sec * 1e3:9.1f} ms = {sec / med['op']:.0f} x the op, counts equal: {same_np}"
            rec["cases"][f"{N}_{mode}"] = case
            out.append(line)
            print(line, flush=True)
        del dist, items, flat
    text = "\n".join(out + [json.dumps(rec)])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
