"""numpy restatement of AEW_OP_SEQ_SEARCH (include/aewavenet.h states the rule; csrc/aew_search.hip implements it).

fp32 throughout, every operation rounded on its own; d(i, j) is AEW_OP_SEQ_ALIGN's local distance
(seq_align_emulator.local_distance).  With a query of n frames and a document of m:
  sweep    C(0,j) = d(0,j), S(0,j) = 1, B(0,j) = j;  for i >= 1: C(i,j) = d(i,j) + C(pred), S(i,j) = S(pred) + 1,
           B(i,j) = B(pred), pred = the existing predecessor of least C among (i-1,j-1), (i-1,j), (i,j-1), ties to the
           first in that order
  profile  (C, S, B)(n-1, j) for every j
  pick     n_hits rounds: the eligible, unsuppressed end of least key (cost / steps or cost), ties to the least j; then
           every end whose interval [B, j] meets the hit's is suppressed
`sweep` runs over anti-diagonals, a diagonal per numpy step; `sweep_loops` is the same rule cell by cell, and the CPU tests
hold the two to each other, to a brute force over all paths and to the closed DTW of seq_align_emulator on slices."""
import numpy as np

from tests.seq_align_emulator import EUCLID, SQEUCLID, F32, local_distance   # noqa: F401  (re-exported)

MEAN, COST = 0, 1
MAX_HITS = 32


def _special(n, m, d):
    """The profile of a pair the sweep does not run for, or None: an empty query (+inf, 0, -1), a non-finite pair
    (NaN, 0, -1); m = 0 owns no entries."""
    if n == 0 or m == 0:
        return np.full(m, np.inf, F32), np.zeros(m, np.int32), np.full(m, -1, np.int32), False
    if not np.isfinite(d).all():
        return np.full(m, np.nan, F32), np.zeros(m, np.int32), np.full(m, -1, np.int32), True
    return None


def sweep(a, b, metric=EUCLID, full=False):
    """-> (end_cost float32 (m,), end_steps int32 (m,), end_start int32 (m,), bad).  full=True: the whole (n, m) C, S, B
    matrices in place of their last rows (ordinary pairs only)."""
    n, m = len(a), len(b)
    d = local_distance(a, b, metric) if n and m else None
    sp = _special(n, m, d)
    if sp is not None:
        return sp
    C = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    B = np.zeros((n, m), np.int64)
    C[0], S[0], B[0] = d[0], 1, np.arange(m)
    with np.errstate(all="ignore"):
        for s in range(1, n + m - 1):
            i = np.arange(max(1, s - m + 1), min(n - 1, s) + 1)               # (row 0 is done)
            if i.size == 0:
                continue
            j = s - i
            has_left = j > 0
            jm = np.maximum(j - 1, 0)
            cd, cu, cl = C[i - 1, jm], C[i - 1, j], C[i, jm]
            # scanning (i-1,j-1), (i-1,j), (i,j-1) with a strict <; at j = 0 only (i-1,j) exists
            t = ~has_left | (cu < cd)
            best = np.where(t, cu, cd)
            bs, bb = np.where(t, S[i - 1, j], S[i - 1, jm]), np.where(t, B[i - 1, j], B[i - 1, jm])
            t = has_left & (cl < best)
            best, bs, bb = np.where(t, cl, best), np.where(t, S[i, jm], bs), np.where(t, B[i, jm], bb)
            C[i, j] = (d[i, j] + best.astype(F32)).astype(F32)
            S[i, j] = bs + 1
            B[i, j] = bb
    if full:
        return C, S, B, False
    return C[n - 1].copy(), S[n - 1].astype(np.int32), B[n - 1].astype(np.int32), False


def sweep_loops(a, b, metric=EUCLID):
    """The same rule cell by cell."""
    n, m = len(a), len(b)
    d = local_distance(a, b, metric) if n and m else None
    sp = _special(n, m, d)
    if sp is not None:
        return sp
    C = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    B = np.zeros((n, m), np.int64)
    for i in range(n):
        for j in range(m):
            if i == 0:
                C[0, j], S[0, j], B[0, j] = d[0, j], 1, j
                continue
            best = None
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
                if pj < 0:
                    continue
                if best is None or C[pi, pj] < best[0]:
                    best = (C[pi, pj], S[pi, pj], B[pi, pj])
            C[i, j] = F32(d[i, j] + best[0])
            S[i, j] = best[1] + 1
            B[i, j] = best[2]
    return C[n - 1].copy(), S[n - 1].astype(np.int32), B[n - 1].astype(np.int32), False


def keys(end_cost, end_steps, rank=MEAN):
    with np.errstate(all="ignore"):
        return (end_cost / end_steps.astype(F32)).astype(F32) if rank == MEAN else end_cost.astype(F32)


def pick(end_cost, end_steps, end_start, n_hits=1, rank=MEAN, min_len=1, max_len=0):
    """-> (hits int32 (n_hits, 2), cost float32 (n_hits,), steps int32 (n_hits,), count).  The slots behind `count` are
    (-1, -1), +inf, 0."""
    m = len(end_cost)
    hits = np.full((n_hits, 2), -1, np.int32)
    cost = np.full(n_hits, np.inf, F32)
    steps = np.zeros(n_hits, np.int32)
    j = np.arange(m)
    key = keys(end_cost, end_steps, rank)
    length = j - end_start + 1
    live = np.isfinite(key) & (length >= min_len)
    if max_len > 0:
        live &= length <= max_len
    count = 0
    for r in range(n_hits):
        if not live.any():
            break
        k = np.where(live, key, np.inf)
        e = int(np.argmin(k))                                                 # (the first of equal keys: the least j)
        s = int(end_start[e])
        hits[r], cost[r], steps[r] = (s, e), end_cost[e], end_steps[e]
        live &= ~((end_start <= e) & (j >= s))
        count += 1
    return hits, cost, steps, count


def search(a, b, metric=EUCLID, n_hits=1, rank=MEAN, min_len=1, max_len=0):
    """One pair from start to end: (profile = (cost, steps, start), hits, hit cost, hit steps, count, bad)."""
    ec, es, eb, bad = sweep(a, b, metric)
    hits, cost, steps, count = pick(ec, es, eb, n_hits, rank, min_len, max_len)
    return (ec, es, eb), hits, cost, steps, count, bad


# ---- the tables align.py builds, restated ---------------------------------------------------------------------------
def prof_bases(lens_b, pairs):
    """(prof_base per pair, n_prof): the prefix sums of the document lengths over the pairs in order."""
    out, at = [], 0
    for _, b in pairs:
        out.append(at)
        at += lens_b[b]
    return out, at


def ws_stride(lens_a, lens_b, pairs):
    """The longest document among the pairs whose query has more than 64 frames (12 * pairs * this bytes of workspace)."""
    return max([lens_b[b] for a, b in pairs if lens_a[a] > 64] or [0])
