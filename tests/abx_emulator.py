"""numpy restatement of AEW_OP_ABX_COUNT and of align.abx_aggregate (include/aewavenet.h states the rule;
csrc/aew_abx.hip and ae_wavenet_amd/align.py implement it).  Nothing here knows the sorted order, the group table or the
partner table: the conditions are written out on the labels of the unsorted items, x by x.

    n, wrong2, cats, spks = counts(D, category, speaker, mode)     # (N, C, S) int64: [item x][category of B][speaker of B]
    error, pooled, by_category, n_triples = aggregate(n, wrong2, category, speaker, mode)
"""
import numpy as np


def index_labels(category, speaker, mode):
    """(ci, si, cats, spks): label indices in order of first appearance; mode "any" gives every item speaker 0."""
    cat = list(category)
    spk = [0] * len(cat) if speaker is None or mode == "any" else list(speaker)
    cats, spks = list(dict.fromkeys(cat)), list(dict.fromkeys(spk))
    return (np.array([cats.index(c) for c in cat]), np.array([spks.index(s) for s in spk]), cats, spks)


def counts(D, category, speaker, mode):
    """For every item x, every category c other than x's and every speaker s the mode allows (within / any: s is x's;
    across: s is not x's): A = the items of x's category under s without x, B = the items of category c under s;
    n = |A| |B|, wrong2 = the sum of 2 [D[x,a] > D[x,b]] + 1 [neither is smaller] over the pairs.  Zero where A or B is
    empty."""
    D = np.asarray(D, np.float32)
    ci, si, cats, spks = index_labels(category, speaker, mode)
    N, C, S = len(ci), len(cats), len(spks)
    n, wrong2 = np.zeros((N, C, S), np.int64), np.zeros((N, C, S), np.int64)
    item = np.arange(N)
    with np.errstate(invalid="ignore"):
        for x in range(N):
            for s in range(S):
                if (s == si[x]) == (mode == "across"):
                    continue
                A = np.flatnonzero((ci == ci[x]) & (si == s) & (item != x))
                if not A.size:
                    continue
                da = D[x, A][:, None]
                for c in range(C):
                    B = np.flatnonzero((ci == c) & (si == s))
                    if c == ci[x] or not B.size:
                        continue
                    db = D[x, B][None, :]
                    gt, lt = da > db, da < db
                    n[x, c, s] = A.size * B.size
                    wrong2[x, c, s] = 2 * int(gt.sum()) + int((~gt & ~lt).sum())
    return n, wrong2, cats, spks


def aggregate(n, wrong2, category, speaker, mode):
    """(error, pooled, by_category (C, C), n_triples) in Python floats / a float64 array: the counts pooled over the x of
    one (category, speaker), a cell's error wrong2 / (2 n), by_category the mean over the (speaker of X, speaker of B)
    combinations that have triples, error the mean over the ordered category pairs that have any.  NaN where nothing is."""
    ci, si, cats, spks = index_labels(category, speaker, mode)
    C, S = len(cats), len(spks)
    by_category = np.full((C, C), np.nan)
    for cx in range(C):
        for cb in range(C):
            errs = []
            for sx in range(S):
                rows = (ci == cx) & (si == sx)
                for sb in range(S):
                    nn, ww = int(n[rows, cb, sb].sum()), int(wrong2[rows, cb, sb].sum())
                    if nn > 0:
                        errs.append(ww / (2.0 * nn))
            if errs:
                by_category[cx, cb] = sum(errs) / len(errs)
    have = ~np.isnan(by_category)
    error = float(by_category[have].sum() / have.sum()) if have.any() else float("nan")
    n_triples = int(n.sum())
    pooled = int(wrong2.sum()) / (2.0 * n_triples) if n_triples else float("nan")
    return error, pooled, by_category, n_triples
