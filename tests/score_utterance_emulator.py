"""Numpy / plain-Python restatement of whole-utterance scoring (include/aewavenet.h: aew_score_row_t, AEW_OP_WAV_TILE,
AEW_OP_NLL_STITCH, AEW_OP_SCORE_REDUCE; ae_wavenet_amd/codes.py: score_tile_plan; geometry.py: scoring_geometry): the hop,
the work list as loops over utterances and windows, the three ops element by element - the reduce in the fixed order of
aew_eval_acc_t -, which codes a conditioning position reads, and a toy causal "decoder" whose per-position value is an
exact float64 hash of the rows it reads, so that "tiles, stitched" and "one run over everything" compare with ==.
Written from the header's text and the issue; shares no code with the package (the conditioning chain itself is
tests/cond_utterance_emulator.py's)."""
import numpy as np

from tests import cond_utterance_emulator as CE

ROW = np.dtype([("code0", "<i8"), ("wav_base", "<i8"), ("wav_len", "<i8"), ("wav0", "<i8"), ("dst", "<i8"), ("utt", "<i4"),
                ("lo", "<i4"), ("hi", "<i4"), ("voice", "<i4"), ("src", "<i4"), ("n_out", "<i4")])


def hop(S, T, rf, trim0):
    """(p, r0, h_s): pad codes in front of window 0, first owned output, hop in codes; the window has w = T - rf outputs
    of which the last carries no loss."""
    p = -(-trim0 // S)
    r0 = p * S - trim0
    return p, r0, (T - rf - 1 - r0) // S


def tile_plan(n_codes, wav_lens, E, S, T, rf, trim0, o, B, L_of):
    """(n_u [U], n_scored [U], offsets [U + 1], rows, n_rows): rows = one dict per batch row - utt (-1 idle), window,
    start (first code of the window relative to the utterance's), lo, hi, wav0, src, n_out, dst - padded with idle rows
    to a multiple of B."""
    p, r0, h_s = hop(S, T, rf, trim0)
    assert h_s >= 1
    n_us, n_sc, offsets, rows = [], [], [0], []
    for u, (N, W) in enumerate(zip(n_codes, wav_lens)):
        n_u = max(min(L_of(N), W - o), 0)
        n = max(n_u - rf - 1, 0)
        n_us.append(n_u)
        n_sc.append(n)
        j = 0
        while j * h_s * S < n:
            c0 = j * h_s - p
            lo = min(max(-c0, 0), E)
            hi = max(min(max(N - c0, 0), E), lo)
            rows.append(dict(utt=u, window=j, start=c0, lo=lo, hi=hi, wav0=o + j * h_s * S - r0, src=r0,
                             n_out=min(h_s * S, n - j * h_s * S), dst=offsets[-1] + j * h_s * S))
            j += 1
        offsets.append(offsets[-1] + n)
    n_rows = len(rows)
    while len(rows) % B:
        rows.append(dict(utt=-1, window=0, start=0, lo=0, hi=0, wav0=0, src=0, n_out=0, dst=0))
    return n_us, n_sc, offsets, rows, n_rows


def table(rows, code_bases, wav_bases, wav_lens, voices):
    rec = np.zeros(len(rows), ROW)
    rec["utt"] = -1
    for k, r in enumerate(rows):
        u = r["utt"]
        if u >= 0:
            rec[k] = (code_bases[u] + r["start"], wav_bases[u], wav_lens[u], r["wav0"], r["dst"], u, r["lo"], r["hi"],
                      voices[u], r["src"], r["n_out"])
    return rec


def wav_tile(tbl, first, B, codes, wavs, E, K, T, n_quant, zero):
    """(wav (B, T) float32, ind (B, E) int64, in_voice (B,) int64, bad_codes, bad_wav): the windows; the zero code / code
    0 where there is nothing or the value lies outside its range - those are counted."""
    wav = np.full((B, T), zero, np.float32)
    ind, voice, bad_c, bad_w = np.zeros((B, E), np.int64), np.zeros(B, np.int64), 0, 0
    for b in range(B):
        r = tbl[first + b]
        if r["utt"] < 0:
            continue
        voice[b] = r["voice"]
        for j in range(int(r["lo"]), int(r["hi"])):
            c = int(codes[int(r["code0"]) + j])
            if 0 <= c < K:
                ind[b, j] = c
            else:
                bad_c += 1
        for t in range(T):
            pos = int(r["wav0"]) + t
            if 0 <= pos < int(r["wav_len"]):
                v = np.float32(wavs[int(r["wav_base"]) + pos])
                if v >= 0 and v < n_quant:                                # (a NaN fails both)
                    wav[b, t] = v
                else:
                    bad_w += 1
    return wav, ind, voice, bad_c, bad_w


def argmax_lowest(logits):
    """The class of the largest value, the lowest one at a tie (strictly-greater scan from class 0)."""
    am, best = 0, logits[0]
    for c in range(1, len(logits)):
        if logits[c] > best:
            best, am = logits[c], c
    return am


def nll_stitch(tbl, first, B, nll, dst_nll, ptgt=None, dst_ptgt=None, amax=None, logits=None, tgt=None, dst_hit=None):
    """In place on the flat outputs: nll / ptgt (B, w) any dtype (bits are moved); the hit from amax (B, w) or from
    logits (B, w, Q), against tgt (B, w) = the target class of every position."""
    for b in range(B):
        r = tbl[first + b]
        if r["utt"] < 0:
            continue
        a, n, d = int(r["src"]), int(r["n_out"]), int(r["dst"])
        dst_nll[d:d + n] = nll[b, a:a + n]
        if dst_ptgt is not None:
            dst_ptgt[d:d + n] = ptgt[b, a:a + n]
        if dst_hit is not None:
            for i in range(n):
                am = int(amax[b, a + i]) if amax is not None else argmax_lowest(logits[b, a + i])
                dst_hit[d + i] = 1 if am == int(tgt[b, a + i]) else 0


def tree_sum(x):
    """sum of float32 / uint8 x in THE order of aew_eval_acc_t: thread t adds elements t, t + 1024, ... ascending into a
    double, then for o = 512, 256, ..., 1: s[t] += s[t + o] for t < o."""
    s = np.zeros(1024, np.float64)
    x = np.asarray(x).astype(np.float64)
    for i0 in range(0, len(x), 1024):                                      # pass k adds element t + 1024 k to thread t
        part = x[i0:i0 + 1024]
        s[:len(part)] = s[:len(part)] + part
    o = 512
    while o > 0:
        s[:o] = s[:o] + s[o:2 * o]
        o >>= 1
    return s[0]


def score_reduce(offsets, nll, ptgt=None, hit=None):
    """(acc (U, 4) float64 = (n, sum nll, sum ptgt, sum hit), out (U, 4) float32 = (nll per sample, bits per sample,
    top-1, mean target probability)): quotients in double, rounded to fp32 once, all 0 where n = 0."""
    U = len(offsets) - 1
    acc, out = np.zeros((U, 4), np.float64), np.zeros((U, 4), np.float32)
    for u in range(U):
        a, b = int(offsets[u]), int(offsets[u + 1])
        n = b - a
        acc[u] = (n, tree_sum(nll[a:b]), tree_sum(ptgt[a:b]) if ptgt is not None else 0.0,
                  tree_sum(hit[a:b] != 0) if hit is not None else 0.0)
        if n > 0:
            m = acc[u, 1] / n
            out[u] = (np.float32(m), np.float32(m / 0.693147180559945309417232121458), np.float32(acc[u, 3] / n),
                      np.float32(acc[u, 2] / n))
    return acc, out


# ---- which codes a conditioning position reads ----------------------------------------------------------------------
def code_span(q, filters, strides):
    """(first, last) code index that row q of the last upsampler's output over a code sequence reads: backwards through
    the transposed convolutions with padding f - s (output row i of a stage reads its input rows m with
    0 <= i + (f - s) - m s < f) and the k = 3 valid LC convolution (row m reads codes m .. m + 2).  No clipping: the chain
    is valid, so for 0 <= q < L(N) the span lies inside [0, N)."""
    lo = hi = q
    for f, s in zip(reversed(filters), reversed(strides)):
        lo = -(-(lo - s + 1) // s)
        hi = (hi + f - s) // s
    return lo, hi + 2


# ---- a toy causal decoder: exact float64 hashes ------------------------------------------------------------------------
def toy_value(cond_rows, wav_rows, target):
    """The value of one output from the rf + 1 cond rows (rf + 1, C) and decoder-input samples (rf + 1,) it reads and
    its target sample: small integer weights, every product and sum exact in float64."""
    k = np.arange(1, len(wav_rows) + 1, dtype=np.float64)
    return float((k[:, None] * cond_rows).sum() + 7.0 * ((k + 1.0) * wav_rows).sum() + 13.0 * target)


def toy_whole(codes, wav, wts, filters, strides, rf, o):
    """One run over the whole utterance: the value of every scored position q_t in [rf + 1, n_u)."""
    cond = CE.chain(codes, wts, filters, strides)
    n_u = max(min(cond.shape[0], len(wav) - o), 0)
    w = np.asarray(wav, np.float64)
    return np.array([toy_value(cond[q - rf - 1:q], w[o + q - rf - 1:o + q], w[o + q]) for q in range(rf + 1, n_u)])


def toy_tiled(codes_list, wavs, wts, filters, strides, E, S, T, rf, trim0, o, B, n_quant=256, zero=128.0):
    """Per utterance the values assembled from windows through the three emulated ops: every batch row's E codes through
    the chain (its T rows from trim0 on are the window's cond), its T samples through wav_tile, the w - 1 outputs that
    carry a loss computed from them, the owned ones stitched.  Returns (list of per-utterance arrays, count list)."""
    L_of = lambda n: CE.length(n, filters, strides)
    n_codes, wav_lens = [len(c) for c in codes_list], [len(w) for w in wavs]
    n_us, n_sc, offsets, rows, n_rows = tile_plan(n_codes, wav_lens, E, S, T, rf, trim0, o, B, L_of)
    code_bases = np.concatenate([[0], np.cumsum(n_codes)])[:-1]
    wav_bases = np.concatenate([[0], np.cumsum(wav_lens)])[:-1]
    tbl = table(rows, code_bases, wav_bases, wav_lens, [0] * len(codes_list))
    codes_flat = np.concatenate([np.asarray(c, np.int64) for c in codes_list]) if sum(n_codes) else np.zeros(0, np.int64)
    wav_flat = np.concatenate([np.asarray(w, np.float32) for w in wavs]) if sum(wav_lens) else np.zeros(0, np.float32)
    w_out = T - rf
    flat = np.full(offsets[-1], np.nan)
    count = np.zeros(offsets[-1], np.int64)
    for first in range(0, len(tbl), B):
        wav, ind, _, bad_c, bad_w = wav_tile(tbl, first, B, codes_flat, wav_flat, E, len(wts["emb"]), T, n_quant, zero)
        assert bad_c == 0 and bad_w == 0
        vals = np.zeros((B, w_out))
        for b in range(B):
            cond = CE.chain(ind[b], wts, filters, strides)[trim0:trim0 + T]
            assert cond.shape[0] == T
            x = wav[b].astype(np.float64)
            for u in range(w_out - 1):
                vals[b, u] = toy_value(cond[u:u + rf + 1], x[u:u + rf + 1], x[u + rf + 1])
        nll_stitch(tbl, first, B, vals, flat)
        ones = np.zeros(offsets[-1], np.int64)
        nll_stitch(tbl, first, B, np.ones((B, w_out), np.int64), ones)
        count += ones
    return [flat[offsets[u]:offsets[u + 1]] for u in range(len(codes_list))], \
        [count[offsets[u]:offsets[u + 1]] for u in range(len(codes_list))]
