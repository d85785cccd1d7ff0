"""TEST INFRASTRUCTURE - numpy restatement of the evaluation accumulator (aew_eval_acc_t, include/aewavenet.h), in the
header's order: thread t of 1024 adds its elements t, t + 1024, ... ascending in double, the 1024 partial sums are
folded by the halving tree, one double addition puts the batch's sum into the record.  Accumulation is meant to agree
with the device bit for bit (IEEE additions only); finalize up to the device's log2 / exp2."""
import numpy as np

T = 1024
ACC_N, OUT_N = 16, 16
OUT_NAMES = ("loss", "nll", "bits_per_sample", "top1", "tprb", "dist", "code_entropy", "code_perplexity", "codes_used",
             "term1", "term2", "term3", "term4", "positions", "batches")
LN2 = 0.693147180559945309417232121458


def tree(part):
    """for (o = 512; o > 0; o >>= 1) s[t] += s[t + o] for t < o; returns s[0]."""
    part = part.copy()
    o = T // 2
    while o > 0:
        part[:o] = part[:o] + part[o:2 * o]
        o >>= 1
    return part[0]


def ordered_sum(x):
    """THE order: x 1-D (any float type) -> double.  Row r of the loop is what every thread adds in its r-th pass."""
    x = np.asarray(x).astype(np.float64)
    part = np.zeros(T, np.float64)
    for r in range(0, x.size, T):
        c = x[r:r + T]
        part[:c.size] = part[:c.size] + c
    return tree(part)


def argmax_lowest(logits):
    """[..., n_quant] -> the lowest class holding the maximum: a later class replaces an earlier one only where it is
    strictly greater (aew_softmax_nll_t.amax's rule)."""
    best = logits[..., 0].copy()
    am = np.zeros(best.shape, np.int32)
    for c in range(1, logits.shape[-1]):
        v = logits[..., c]
        m = v > best
        best = np.where(m, v, best)
        am = np.where(m, np.int32(c), am)
    return am


def targets(wav, tgt_off, w):
    """wav [B][wav_pitch] float-encoded ints -> int [B][w - 1]: target[b][u] = (int)wav[b][tgt_off + u + 1]."""
    return wav[:, tgt_off + 1: tgt_off + w].astype(np.int32)


def accumulate(acc, hist, nll, ptgt, wav, tgt_off, amax=None, logits=None, n_quant=None, ind=None, dist=None, loss=None):
    """One batch into (acc float64 [16], hist uint32 [K] or None), in place.  nll / ptgt / amax [B][w]; logits
    [B][w][>= n_quant] (used when amax is None); ind int64 [Q] / dist [Q] optional; loss [5] optional."""
    B, w = nll.shape
    live = slice(0, w - 1)
    am = amax[:, live] if amax is not None else argmax_lowest(logits[:, live, :n_quant])
    hit = (am == targets(wav, tgt_off, w)).astype(np.float32)
    acc[0] += 1.0
    acc[1] += float(B * (w - 1))
    acc[2] += ordered_sum(nll[:, live].reshape(-1))
    acc[3] += ordered_sum(ptgt[:, live].reshape(-1))
    acc[4] += ordered_sum(hit.reshape(-1))
    if ind is not None:
        acc[5] += float(ind.size)
        acc[6] += ordered_sum(dist) if dist is not None else 0.0
        K = hist.size
        ok = (ind >= 0) & (ind < K)
        np.add.at(hist, ind[ok], np.uint32(1))
    if loss is not None:
        acc[7] += np.float64(loss[0])
        for j in range(4):
            acc[8 + j] += np.float64(loss[1 + j])
    return acc, hist


def finalize(acc, hist=None):
    """-> float32 [16] (OUT_NAMES, then 0)."""
    div = lambda x, y: x / y if y > 0.0 else 0.0
    out = np.zeros(OUT_N, np.float32)
    nb, npos, nq = acc[0], acc[1], acc[5]
    nll = div(acc[2], npos)
    out[0] = div(acc[7], nb)
    out[1] = nll
    out[2] = nll / LN2
    out[3] = div(acc[4], npos)
    out[4] = div(acc[3], npos)
    out[5] = div(acc[6], nq)
    if hist is not None:
        h = hist.astype(np.uint64)
        total = int(h.sum())
        if total > 0:
            part = np.zeros(T, np.float64)
            for r in range(0, h.size, T):                            # thread t: codes t, t + 1024, ... ascending
                c = h[r:r + T].astype(np.float64)
                pr = c / float(total)
                term = np.where(c > 0, pr * np.log2(np.where(c > 0, pr, 1.0)), 0.0)
                part[:c.size] = part[:c.size] - term
            ent = tree(part)
            out[6], out[7] = ent, np.exp2(ent)
        out[8] = float((h > 0).sum())
    for j in range(4):
        out[9 + j] = div(acc[8 + j], nb)
    out[13], out[14] = npos, nb
    return out
