"""numpy restatement of AEW_OP_SEQ_ALIGN (include/aewavenet.h states the rule; csrc/aew_align.hip implements it).

fp32 throughout, every operation rounded on its own:
  local distance  acc = 0; for k: t = a[i][k] - b[j][k]; acc = acc + t * t;  d = acc (sqeuclid) or sqrt(acc) (euclid)
  DTW             C(0,0) = d(0,0), S(0,0) = 1; C(i,j) = d(i,j) + C(pred), S(i,j) = S(pred) + 1, pred = the existing
                  predecessor of least C among (i-1,j-1), (i-1,j), (i,j-1), ties to the first in that order
  EDIT            unit-cost Levenshtein distance
The dynamic programme runs over anti-diagonals (every cell of one depends only on the two before it), which lets numpy
take a diagonal at a time; `dtw_loops` is the same rule as plain loops, cell by cell, and the CPU tests hold the two to
each other and to definitions that share no code with either."""
import numpy as np

F32 = np.float32
EUCLID, SQEUCLID = 0, 1


def local_distance(a, b, metric=EUCLID):
    """a (n, D), b (m, D) float32 -> d (n, m) float32 under the rule."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    with np.errstate(all="ignore"):
        for k in range(a.shape[1]):
            t = (a[:, k][:, None] - b[:, k][None, :]).astype(F32)
            acc = (acc + (t * t).astype(F32)).astype(F32)
        return acc if metric == SQEUCLID else np.sqrt(acc).astype(F32)


def dtw(a, b, metric=EUCLID, want_back=False):
    """-> (cost float32, steps int, back uint8 (n, m) or None).  An empty side: (+inf, 0); any non-finite d: (NaN, 0)."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return F32(np.inf), 0, None
    d = local_distance(a, b, metric)
    if not np.isfinite(d).all():
        return F32(np.nan), 0, (np.zeros((n, m), np.uint8) if want_back else None)
    C = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    back = np.zeros((n, m), np.uint8)
    C[0, 0], S[0, 0] = d[0, 0], 1
    with np.errstate(all="ignore"):
        for s in range(1, n + m - 1):
            i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
            j = s - i
            has_up, has_left = i > 0, j > 0
            im, jm = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            cd, cu, cl = C[im, jm], C[im, j], C[i, jm]
            sd, su, sl = S[im, jm], S[im, j], S[i, jm]
            both = has_up & has_left
            # scanning (i-1,j-1), (i-1,j), (i,j-1) with a strict <
            best, bs, which = cd.copy(), sd.copy(), np.zeros(i.size, np.uint8)
            t = both & (cu < best)
            best, bs, which = np.where(t, cu, best), np.where(t, su, bs), np.where(t, 1, which)
            t = both & (cl < best)
            best, bs, which = np.where(t, cl, best), np.where(t, sl, bs), np.where(t, 2, which)
            only_up, only_left = has_up & ~has_left, has_left & ~has_up
            best, bs, which = np.where(only_up, cu, best), np.where(only_up, su, bs), np.where(only_up, 1, which)
            best, bs, which = np.where(only_left, cl, best), np.where(only_left, sl, bs), np.where(only_left, 2, which)
            C[i, j] = (d[i, j] + best.astype(F32)).astype(F32)
            S[i, j] = bs + 1
            back[i, j] = which
    return C[n - 1, m - 1], int(S[n - 1, m - 1]), (back if want_back else None)


def dtw_loops(a, b, metric=EUCLID):
    """The same rule cell by cell: (cost, steps, back)."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return F32(np.inf), 0, None
    d = local_distance(a, b, metric)
    if not np.isfinite(d).all():
        return F32(np.nan), 0, None
    C = np.zeros((n, m), F32)
    S = np.zeros((n, m), np.int64)
    back = np.zeros((n, m), np.uint8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                C[0, 0], S[0, 0] = d[0, 0], 1
                continue
            best = None
            for which, (pi, pj) in enumerate(((i - 1, j - 1), (i - 1, j), (i, j - 1))):
                if pi < 0 or pj < 0:
                    continue
                if best is None or C[pi, pj] < best[0]:
                    best = (C[pi, pj], S[pi, pj], which)
            C[i, j] = F32(d[i, j] + best[0])
            S[i, j] = best[1] + 1
            back[i, j] = best[2]
    return C[n - 1, m - 1], int(S[n - 1, m - 1]), back


def walk(back, steps):
    """The path the second kernel writes: (n + m - 1, 2) int32, the `steps` cells from (0,0) to (n-1,m-1), then (-1,-1)."""
    n, m = back.shape
    out = np.full((n + m - 1, 2), -1, np.int32)
    i, j = n - 1, m - 1
    for e in range(steps - 1, -1, -1):
        out[e] = (i, j)
        w = int(back[i, j])
        if w != 2:
            i -= 1
        if w != 1:
            j -= 1
        i, j = max(i, 0), max(j, 0)
    return out


def edit(a, b):
    """Unit-cost Levenshtein distance of two integer sequences (row by row, one numpy scan per row)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    n, m = a.size, b.size
    if n == 0 or m == 0:
        return n + m
    prev = np.arange(m + 1, dtype=np.int64)
    for i in range(n):
        sub = prev[:-1] + (b != a[i])
        base = np.minimum(sub, prev[1:] + 1)                  # without the left neighbour
        cur = np.empty(m + 1, np.int64)
        cur[0] = i + 1
        # cur[j+1] = min(base[j], cur[j] + 1): a running minimum of base[j] - j, shifted back
        run = np.minimum.accumulate(np.concatenate([[cur[0]], base - np.arange(1, m + 1)]))
        cur[1:] = np.minimum(base, run[:-1] + np.arange(1, m + 1))
        prev = cur
    return int(prev[m])


# ---- the tables align.py builds, restated ---------------------------------------------------------------------------
def pair_bases(lens_a, lens_b, pairs):
    """(back_base, path_base, n_back, n_path): prefix sums of n * m bytes and n + m - 1 entries over the pairs in order;
    a pair with an empty side owns nothing."""
    bb, pb, nb, npth = [], [], 0, 0
    for a, b in pairs:
        n, m = lens_a[a], lens_b[b]
        bb.append(nb)
        pb.append(npth)
        if n and m:
            nb += n * m
            npth += n + m - 1
    return bb, pb, nb, npth


def chunks(lens_a, lens_b, pairs, max_back_bytes):
    """[(first pair, one past the last)]: consecutive pairs whose back matrices fit max_back_bytes together; a pair
    larger than that on its own gets a launch of its own."""
    out, lo, held = [], 0, 0
    for p, (a, b) in enumerate(pairs):
        cells = lens_a[a] * lens_b[b]
        if p > lo and held + cells > max_back_bytes:
            out.append((lo, p))
            lo, held = p, 0
        held += cells
    if len(pairs) > lo:
        out.append((lo, len(pairs)))
    return out
