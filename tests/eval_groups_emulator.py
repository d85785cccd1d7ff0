"""TEST INFRASTRUCTURE - numpy restatement of the grouped evaluation accumulator (aew_eval_groups_t,
include/aewavenet.h), in the header's order: per window THE order and THE tree of tests/eval_emulator.py, per group the
windows ascending with one double addition per entry.  Accumulation is meant to agree with the device bit for bit (IEEE
additions only); finalize up to the device's log2 / exp2."""
import numpy as np

from tests.eval_emulator import LN2, T, argmax_lowest, ordered_sum, targets, tree

GACC_N, GOUT_N, TOUT_N = 8, 12, 16
GOUT_NAMES = ("windows", "positions", "nll", "bits_per_sample", "top1", "tprb", "dist", "queries", "code_entropy",
              "code_perplexity", "codes_used")
TOUT_NAMES = ("n", "code_entropy", "group_entropy", "cond_entropy", "mutual_information", "mutual_information_mm",
              "mi_over_group_entropy", "mi_over_code_entropy", "cells", "groups_used", "codes_used", "dropped_windows",
              "batches")


def new_record(G, K, B):
    """(gacc, ghist or None, gtot, win), zeroed."""
    return (np.zeros((G, GACC_N)), np.zeros((G, K), np.uint32) if K else None, np.zeros(4), np.zeros((B, 4)))


def accumulate(gacc, ghist, gtot, win, group, nll=None, ptgt=None, wav=None, tgt_off=0, amax=None, logits=None,
               n_quant=None, ind=None, dist=None):
    """One batch into the record, in place.  nll / ptgt / amax [B][w] (nll None: codes-only); logits [B][w][>= n_quant]
    (used when amax is None); ind int64 [B][Qw] / dist [B][Qw] optional; group int64 [B]."""
    G = gacc.shape[0]
    B = group.size
    win[:] = 0.0
    if nll is not None:
        w = nll.shape[1]
        live = slice(0, w - 1)
        am = amax[:, live] if amax is not None else argmax_lowest(logits[:, live, :n_quant])
        hit = (am == targets(wav, tgt_off, w)).astype(np.float32)
        for b in range(B):
            win[b, 0], win[b, 1], win[b, 2] = ordered_sum(nll[b, live]), ordered_sum(ptgt[b, live]), ordered_sum(hit[b])
    if ind is not None:
        ind = ind.reshape(B, -1)
        K = ghist.shape[1]
        for b in range(B):
            if dist is not None:
                win[b, 3] = ordered_sum(dist.reshape(B, -1)[b])
            if 0 <= group[b] < G:
                ok = (ind[b] >= 0) & (ind[b] < K)
                np.add.at(ghist[group[b]], ind[b][ok], np.uint32(1))
    for b in range(B):                                              # thread g walks b ascending: per entry, this order
        g = int(group[b])
        if not 0 <= g < G:
            gtot[0] += 1.0
            continue
        gacc[g, 0] += 1.0
        if nll is not None:
            gacc[g, 1] += float(nll.shape[1] - 1)
            gacc[g, 2] += win[b, 0]
            gacc[g, 3] += win[b, 1]
            gacc[g, 4] += win[b, 2]
        if ind is not None:
            gacc[g, 5] += float(ind.shape[1])
            if dist is not None:
                gacc[g, 6] += win[b, 3]
    gtot[1] += 1.0
    return gacc, ghist, gtot, win


def _strided(terms):
    """THE order over k for a [K] array of double terms (zeros where a term is skipped), then THE tree."""
    part = np.zeros(T, np.float64)
    for r in range(0, terms.size, T):
        c = terms[r:r + T]
        part[:c.size] = part[:c.size] + c
    return tree(part)


def _plogp(c, total):
    """-p log2 p per entry with p = c / total (double), 0 where c == 0."""
    c = c.astype(np.float64)
    pr = c / float(total)
    return -np.where(c > 0, pr * np.log2(np.where(c > 0, pr, 1.0)), 0.0)


def finalize(gacc, ghist, gtot):
    """-> (gout float32 [G][12], tout float32 [16]): finalize64 rounded to fp32 once."""
    gout, tout = finalize64(gacc, ghist, gtot)
    return gout.astype(np.float32), tout.astype(np.float32)


def finalize64(gacc, ghist, gtot):
    """The doubles the device rounds: (gout float64 [G][12], tout float64 [16])."""
    div = lambda x, y: x / y if y > 0.0 else 0.0
    G = gacc.shape[0]
    gout, tout = np.zeros((G, GOUT_N), np.float64), np.zeros(TOUT_N, np.float64)
    rows = np.zeros((G, 4))
    if ghist is not None:
        h = ghist.astype(np.uint64)
        cols = h.sum(0)
        N = int(cols.sum())
    for g in range(G):
        a = gacc[g]
        nll = div(a[2], a[1])
        gout[g, 0], gout[g, 1], gout[g, 2], gout[g, 3] = a[0], a[1], nll, nll / LN2
        gout[g, 4], gout[g, 5], gout[g, 6], gout[g, 7] = div(a[4], a[1]), div(a[3], a[1]), div(a[6], a[5]), a[5]
        if ghist is None:
            continue
        n_g = int(h[g].sum())
        cells = float((h[g] > 0).sum())
        ent = J = 0.0
        if n_g > 0:
            ent = _strided(_plogp(h[g], n_g))
            c = h[g].astype(np.float64)
            nz = c > 0
            ratio = np.where(nz, (c * float(N)) / np.where(nz, float(n_g) * cols.astype(np.float64), 1.0), 1.0)
            J = _strided(np.where(nz, c * np.log2(ratio), 0.0))
            gout[g, 9] = np.exp2(ent)
        gout[g, 8], gout[g, 10] = ent, cells
        rows[g] = n_g, ent, J, cells
    tout[11], tout[12] = gtot[0], gtot[1]
    if ghist is None:
        return gout, tout
    hc = _strided(_plogp(cols, N)) if N > 0 else 0.0
    n_cols = float((cols > 0).sum())
    hg = hcg = jsum = cells = n_rows = 0.0
    for g in range(G):                                              # ascending g, one thread
        if not rows[g, 0] > 0.0:
            continue
        pg = rows[g, 0] / float(N)
        hg -= pg * np.log2(pg)
        hcg += pg * rows[g, 1]
        jsum += rows[g, 2]
        cells += rows[g, 3]
        n_rows += 1.0
    mi = div(jsum, float(N))
    mm = mi - (cells - n_rows - n_cols + 1.0) / (2.0 * float(N) * LN2) if N > 0 else 0.0
    tout[:11] = float(N), hc, hg, hcg, mi, mm, div(mi, hg), div(mi, hc), cells, n_rows, n_cols
    return gout, tout
