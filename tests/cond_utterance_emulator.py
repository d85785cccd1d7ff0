"""Numpy / plain-Python restatement of whole-utterance conditioning (include/aewavenet.h: aew_cond_row_t,
AEW_OP_CODE_TILE, AEW_OP_COND_STITCH; ae_wavenet_amd/codes.py: cond_tile_plan; geometry.py: conditioning_geometry): the
length recurrence, the work list as loops over utterances and windows, the two ops element by element, and a float64
emulator of the conditioning chain itself - lookup, k = 3 valid convolution, transposed convolutions with padding f - s -
whose sums are exact for small integer weights, so that "tiles, stitched" and "one run over everything" compare with ==.
Written from the header's text and the issue; shares no code with the package."""
import numpy as np

ROW = np.dtype([("code0", "<i8"), ("utt", "<i4"), ("stream", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("src_row", "<i4"),
                ("n_rows", "<i4"), ("dst_row", "<i4"), ("pitch", "<i4"), ("voice", "<i4"), ("first", "<i4")])

REF_FILTERS, REF_STRIDES = (25, 16, 16, 16), (5, 4, 4, 4)
CASES = (6, 7, 9, 10, 11, 12, 17)                       # the issue's utterances, in codes


def length(n, filters, strides):
    """L(n): rows behind the last upsampler for n codes; 0 where the recurrence goes non-positive."""
    n = n - 2
    for f, s in zip(filters, strides):
        if n < 1:
            return 0
        n = (n + 1) * s - f
    return max(n, 0)


def hop(S, T, trim0):
    """(p, lead, h): pad codes in front of window 0, first owned cond row, hop in codes."""
    p = -(-trim0 // S)
    lead = p * S - trim0
    return p, lead, (T - lead) // S


def tile_plan(n_codes, E, S, T, trim0, B, L_of):
    """(lengths [U], pitch, rows, n_rows): rows = one dict per batch row - utt (-1 idle), window, start (first code of
    the window relative to the utterance's), lo, hi, src_row, n_rows, dst_row, first - padded with idle rows to a multiple
    of B."""
    p, lead, h = hop(S, T, trim0)
    assert h >= 1
    lengths, rows = [], []
    for u, N in enumerate(n_codes):
        Ln = L_of(N)
        lengths.append(Ln)
        w = 0
        while w * h * S < Ln:
            c0 = w * h - p
            lo = min(max(-c0, 0), E)
            hi = max(min(max(N - c0, 0), E), lo)
            rows.append(dict(utt=u, window=w, start=c0, lo=lo, hi=hi, src_row=lead, n_rows=min(h * S, Ln - w * h * S),
                             dst_row=w * h * S, first=int(w == 0)))
            w += 1
    n_rows = len(rows)
    while len(rows) % B:
        rows.append(dict(utt=-1, window=0, start=0, lo=0, hi=0, src_row=0, n_rows=0, dst_row=0, first=0))
    return lengths, max(max(lengths, default=0), 1), rows, n_rows


def table(rows, bases, voices, pitch):
    rec = np.zeros(len(rows), ROW)
    rec["utt"] = -1
    for k, r in enumerate(rows):
        u = r["utt"]
        if u >= 0:
            rec[k] = (bases[u] + r["start"], u, u, r["lo"], r["hi"], r["src_row"], r["n_rows"], r["dst_row"], pitch,
                      voices[u], r["first"])
    return rec


def code_tile(tbl, first, B, codes, E, K):
    """(ind (B, E) int64, in_voice (B,) int64, bad): the window codes, 0 where there is none or the code lies outside
    [0, K) - those are counted."""
    ind, voice, bad = np.zeros((B, E), np.int64), np.zeros(B, np.int64), 0
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
                bad += 1
    return ind, voice, bad


def cond_stitch(tbl, first, B, cond, cond_utt, bias, bias_utt):
    """In place on cond_utt (streams, pitch, Cp) and bias_utt (streams, bias_n): cond (B, T, Cp), bias (B, bias_n), any
    dtype (bits are moved)."""
    for b in range(B):
        r = tbl[first + b]
        if r["utt"] < 0:
            continue
        s, n, a, d = int(r["stream"]), int(r["n_rows"]), int(r["src_row"]), int(r["dst_row"])
        cond_utt[s, d:d + n] = cond[b, a:a + n]
        if r["first"]:
            bias_utt[s] = bias[b]


# ---- the chain in float64 ---------------------------------------------------------------------------------------------
def small_weights(filters, K, d, C, seed):
    """Integer-valued float64 weights: codebook (K, d), LC conv (3, d, C), one (f, C, C) per upsampler, biases (C,).
    Entries in [-2, 2]: every sum of the chain stays far below 2^53, so float64 adds them exactly in any order."""
    rs = np.random.RandomState(seed)
    r = lambda *shape: rs.randint(-2, 3, shape).astype(np.float64)
    return dict(emb=r(K, d), lc=r(3, d, C), lc_b=r(C), ups=[r(f, C, C) for f in filters], ups_b=[r(C) for _ in filters])


def chain(codes, wts, filters, strides):
    """codes (n,) -> the last upsampler's output (L(n), C): emb[codes], the valid k = 3 convolution, then per stage the
    transposed convolution out[i * s + k - (f - s)] += x[i] @ W[k] kept on [0, (n + 1) * s - f)."""
    x = wts["emb"][np.asarray(codes, np.int64)]
    n = x.shape[0] - 2
    if n < 1:
        return np.zeros((0, wts["lc"].shape[2]))
    x = sum(x[k:k + n] @ wts["lc"][k] for k in range(3)) + wts["lc_b"]
    for f, s, W, b in zip(filters, strides, wts["ups"], wts["ups_b"]):
        n = x.shape[0]
        n_out = (n + 1) * s - f
        if n_out < 1:
            return np.zeros((0, W.shape[2]))
        full = np.zeros(((n - 1) * s + f, W.shape[2]))
        for k in range(f):
            full[k:k + (n - 1) * s + 1:s] += x @ W[k]
        x = full[f - s:f - s + n_out] + b
    return x


def tiled(codes_list, wts, filters, strides, E, S, T, trim0, B):
    """Per utterance the conditioning (L(N), C) assembled from windows: every batch row's E codes through chain(), its T
    rows from trim0 on as the window's cond, the owned rows to their place.  count[u][q] = how often position q was
    written."""
    L_of = lambda n: length(n, filters, strides)
    lengths, pitch, rows, n_rows = tile_plan([len(c) for c in codes_list], E, S, T, trim0, B, L_of)
    assert trim0 + T <= L_of(E)
    C = wts["lc"].shape[2]
    out = [np.full((n, C), np.nan) for n in lengths]
    count = [np.zeros(n, np.int64) for n in lengths]
    for r in rows:
        u = r["utt"]
        if u < 0:
            assert r["n_rows"] == 0
            continue
        win = np.zeros(E, np.int64)
        for j in range(r["lo"], r["hi"]):
            win[j] = codes_list[u][r["start"] + j]
        cond = chain(win, wts, filters, strides)[trim0:trim0 + T]
        assert cond.shape[0] == T and 0 <= r["src_row"] and r["src_row"] + r["n_rows"] <= T
        d, n, a = r["dst_row"], r["n_rows"], r["src_row"]
        assert 0 <= d and d + n <= lengths[u]
        out[u][d:d + n] = cond[a:a + n]
        count[u][d:d + n] += 1
    return out, count
