"""numpy restatement of AEW_OP_SEQ_DISCOVER (include/aewavenet.h states the rule; csrc/aew_discover.hip implements it).

fp32 throughout, every operation rounded on its own; d(i, j) is AEW_OP_SEQ_ALIGN's local distance
(seq_align_emulator.local_distance).  With a of n frames, b of m, a finite threshold and a band >= 0:
  gain     g(i,j) = threshold - d(i,j)
  dead     band > 0 and j - i < band: outside the band, H = 0, S = 0
  sweep    inside the band: pred = the predecessor of largest H among (i-1,j-1), (i-1,j), (i,j-1) that exist and have H > 0,
           ties to the first in that order; with one H = H(pred) + g, S = S(pred) + 1, O = O(pred); without one H = g, S = 1,
           O = (i, j); a result that is not > 0 is dead: H = 0, S = 0
  profile  per ROW i: E(i) = max_j H(i,j) with the least such j, that cell's column, origin row, origin column and steps;
           E(i) = 0: (0, -1, -1, -1, 0)
  pick     n_hits rounds: the eligible, unsuppressed row of largest E, ties to the least i; then every row whose own
           A range [origin row, i] meets the hit's is suppressed
`sweep` runs over anti-diagonals, a diagonal per numpy step; `sweep_loops` is the same rule cell by cell, and the CPU tests
hold the two to each other and to a brute force over all paths."""
import numpy as np

from tests.seq_align_emulator import EUCLID, SQEUCLID, F32, local_distance   # noqa: F401  (re-exported)

MAX_HITS = 32


def inside(n, m, band):
    """(n, m) bool: the cells inside the band."""
    i, j = np.arange(n)[:, None], np.arange(m)[None, :]
    return np.ones((n, m), bool) if band <= 0 else (j - i >= band)


def _special(n, m, d, band):
    """The profile of a pair the sweep does not run for, or None: an empty side (0, -1, -1, -1, 0) per row, a pair that is
    not finite inside its band (NaN, -1, -1, -1, 0); n = 0 owns no entries."""
    minus = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return np.zeros(n, F32), minus, minus.copy(), minus.copy(), np.zeros(n, np.int32), False
    if not np.isfinite(d[inside(n, m, band)]).all():
        return np.full(n, np.nan, F32), minus, minus.copy(), minus.copy(), np.zeros(n, np.int32), True
    return None


def _profile(H, S, R, O):
    n = H.shape[0]
    e = H.max(axis=1)
    j = H.argmax(axis=1)                                                      # (the first of equal values: the least j)
    rows = np.arange(n)
    some = e > 0
    pick = lambda x, none: np.where(some, x[rows, j], none).astype(np.int32)
    return (e.astype(F32), np.where(some, j, -1).astype(np.int32), pick(R, -1), pick(O, -1), pick(S, 0))


def sweep(a, b, threshold, metric=EUCLID, band=0, full=False):
    """-> (score float32 (n,), end int32 (n,), origin_row int32 (n,), origin_col int32 (n,), steps int32 (n,), bad).
    full=True: the whole (n, m) H, S, R, O matrices and bad (ordinary pairs only)."""
    n, m = len(a), len(b)
    theta = F32(threshold)
    d = local_distance(a, b, metric) if n and m else None
    sp = _special(n, m, d, band)
    if sp is not None:
        return sp
    live = inside(n, m, band)
    H = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    R = np.zeros((n, m), np.int64)
    O = np.zeros((n, m), np.int64)
    with np.errstate(all="ignore"):
        g = (theta - d).astype(F32)
        for s in range(n + m - 1):
            i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
            j = s - i
            im, jm = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            zero = np.zeros(i.size, F32)
            # a predecessor that does not exist counts as H = 0: never taken
            hd = np.where((i > 0) & (j > 0), H[im, jm], zero)
            hu = np.where(i > 0, H[im, j], zero)
            hl = np.where(j > 0, H[i, jm], zero)
            best, bs, br, bo = hd, S[im, jm], R[im, jm], O[im, jm]
            t = hu > best
            best, bs, br, bo = np.where(t, hu, best), np.where(t, S[im, j], bs), np.where(t, R[im, j], br), np.where(t, O[im, j], bo)
            t = hl > best
            best, bs, br, bo = np.where(t, hl, best), np.where(t, S[i, jm], bs), np.where(t, R[i, jm], br), np.where(t, O[i, jm], bo)
            has = best > 0
            h = np.where(has, (best + g[i, j]).astype(F32), g[i, j]).astype(F32)
            alive = live[i, j] & (h > 0)
            H[i, j] = np.where(alive, h, zero)
            S[i, j] = np.where(alive, np.where(has, bs + 1, 1), 0)
            R[i, j] = np.where(has, br, i)
            O[i, j] = np.where(has, bo, j)
    if full:
        return H, S, R, O, False
    return _profile(H, S, R, O) + (False,)


def sweep_loops(a, b, threshold, metric=EUCLID, band=0, full=False):
    """The same rule cell by cell."""
    n, m = len(a), len(b)
    theta = F32(threshold)
    d = local_distance(a, b, metric) if n and m else None
    sp = _special(n, m, d, band)
    if sp is not None:
        return sp
    H = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    R = np.zeros((n, m), np.int64)
    O = np.zeros((n, m), np.int64)
    for i in range(n):
        for j in range(m):
            R[i, j], O[i, j] = i, j
            if band > 0 and j - i < band:
                continue                                                      # dead: H = 0, S = 0
            g = F32(theta - d[i, j])
            best = None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pi < 0 or pj < 0 or not H[pi, pj] > 0:
                    continue
                if best is None or H[pi, pj] > H[best]:
                    best = (pi, pj)
            if best is None:
                h, st = g, 1
            else:
                h, st = F32(H[best] + g), S[best] + 1
                R[i, j], O[i, j] = R[best], O[best]
            if h > 0:
                H[i, j], S[i, j] = h, st
    if full:
        return H, S, R, O, False
    return _profile(H, S, R, O) + (False,)


def pick(score, end, row, col, steps, n_hits=3, min_len=1, max_len=0):
    """-> (hits int32 (n_hits, 4) = (a_start, a_end, b_start, b_end), score float32 (n_hits,), steps int32 (n_hits,),
    count).  The slots behind `count` are (-1, -1, -1, -1), NaN, 0."""
    n = len(score)
    hits = np.full((n_hits, 4), -1, np.int32)
    hs = np.full(n_hits, np.nan, F32)
    hst = np.zeros(n_hits, np.int32)
    i = np.arange(n)
    la, lb = i - row + 1, end - col + 1
    with np.errstate(invalid="ignore"):
        live = (score > 0) & (la >= min_len) & (lb >= min_len)
    if max_len > 0:
        live &= (la <= max_len) & (lb <= max_len)
    count = 0
    for r in range(n_hits):
        if not live.any():
            break
        e = int(np.argmax(np.where(live, score, -np.inf)))                    # (the first of equal scores: the least i)
        s = int(row[e])
        hits[r], hs[r], hst[r] = (s, e, col[e], end[e]), score[e], steps[e]
        live &= ~((row <= e) & (i >= s))
        count += 1
    return hits, hs, hst, count


def discover(a, b, threshold, metric=EUCLID, band=0, n_hits=3, min_len=1, max_len=0):
    """One pair from start to end: (profile = (score, end, row, col, steps), hits, hit score, hit steps, count, bad)."""
    *prof, bad = sweep(a, b, threshold, metric, band)
    hits, hs, hst, count = pick(*prof, n_hits=n_hits, min_len=min_len, max_len=max_len)
    return tuple(prof), hits, hs, hst, count, bad


# ---- the tables align.py builds, restated ---------------------------------------------------------------------------
def prof_bases(lens_a, pairs):
    """(prof_base per pair, n_prof): the prefix sums of the A lengths over the pairs in order."""
    out, at = [], 0
    for a, _ in pairs:
        out.append(at)
        at += lens_a[a]
    return out, at


def ws_stride(lens_a, lens_b, pairs):
    """The longest B side among the pairs whose A side has more than 64 frames (16 * pairs * this bytes of workspace)."""
    return max([lens_b[b] for a, b in pairs if lens_a[a] > 64] or [0])
