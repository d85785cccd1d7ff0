"""AEW_OP_CODE_SEGMENT restated in numpy fp32 (include/aewavenet.h states the rule): penalised Viterbi decoding of one
utterance's frames over the K codebook entries with a uniform switch cost, independent of the C++ twin.  The local costs
come from the oracle's exact chain, one codebook entry at a time - never from a float64 restatement of the fma, which
would round twice."""
import itertools

import numpy as np

from oracle import exact

F32 = np.float32
INF = F32(np.inf)


def _chain_nonfinite(z, e, metric):
    """c for a (frame, entry) pair whose value is not finite: the chain in float64 steps rounded to fp32 - the rounding
    of a finite step does not decide between inf and NaN."""
    with np.errstate(all="ignore"):
        dd = qq = zz = F32(0)
        for j in range(len(z)):
            u = F32(z[j] - e[j])
            dd = F32(np.float64(u) * np.float64(u) + np.float64(dd))
            qq = F32(np.float64(e[j]) * np.float64(e[j]) + np.float64(qq))
            zz = F32(np.float64(z[j]) * np.float64(z[j]) + np.float64(zz))
        v = dd if metric == "sq_l2" else F32(np.sqrt(dd) / F32(np.sqrt(zz) + np.sqrt(qq)))
    assert not np.isfinite(v)
    return v


def local_costs(frames, emb, metric):
    """(T, K) fp32: c(t, k), column k = the distances exact.vq_nearest reports against the one-entry codebook emb[k].  That
    search starts from +inf and takes a value only if it is below, so a NaN comes back as +inf: those cells are redone."""
    frames, emb = np.ascontiguousarray(frames, F32), np.ascontiguousarray(emb, F32)
    T, K = len(frames), len(emb)
    c = np.empty((T, K), F32)
    if T == 0:
        return c
    for k in range(K):
        c[:, k] = exact.vq_nearest(frames, emb[k:k + 1], metric)[1]
    for t, k in zip(*np.nonzero(np.isinf(c))):
        c[t, k] = _chain_nonfinite(frames[t], emb[k], metric)
    return c


def _min(r):
    """(m, a): strict '<' over ascending k from (+inf, 0) - the lowest index among ties, a NaN never wins."""
    rr = np.where(np.isnan(r), INF, r)
    a = int(np.argmin(rr))                                  # the first occurrence of the minimum
    return (r[a], a) if rr[a] < INF else (INF, 0)


def viterbi(c, lam):
    """The recurrence and the walk back over given local costs c (T, K) fp32 -> dict(codes int64 (T,), dist fp32 (T,), cost
    fp32, n_seg int)."""
    c = np.asarray(c, F32)
    T, K = c.shape
    lam = F32(lam)
    assert lam >= 0
    if T == 0:
        return dict(codes=np.zeros(0, np.int64), dist=np.zeros(0, F32), cost=F32(0), n_seg=0)
    stay = np.zeros((T, K), bool)
    A = np.zeros(T, np.int64)
    r, acc = c[0].copy(), F32(0)
    with np.errstate(all="ignore"):
        for t in range(1, T):
            m, a = _min(r)
            A[t - 1], acc = a, F32(acc + m)
            p = (r - m).astype(F32)
            stay[t] = p < lam
            r = (c[t] + np.where(stay[t], p, lam).astype(F32)).astype(F32)
        m, k = _min(r)
        cost = F32(acc + m)
    codes = np.zeros(T, np.int64)
    for t in range(T - 1, 0, -1):
        codes[t] = k
        if not stay[t, k]:
            k = int(A[t - 1])
    codes[0] = k
    return dict(codes=codes, dist=c[np.arange(T), codes], cost=cost, n_seg=1 + int((codes[1:] != codes[:-1]).sum()))


def segment(frames, emb, metric, lam):
    return viterbi(local_costs(frames, emb, metric), lam)


def segment_ragged(frames, offsets, emb, metric, lams):
    """Utterance u = rows offsets[u] .. offsets[u + 1] of `frames` with penalty lams[u] -> (codes, dist, cost (U,),
    n_seg (U,), n_bad): what one AEW_OP_CODE_SEGMENT leaves."""
    U = len(offsets) - 1
    c = local_costs(frames, emb, metric)
    codes, dist = np.zeros(len(frames), np.int64), np.zeros(len(frames), F32)
    cost, n_seg = np.zeros(U, F32), np.zeros(U, np.int32)
    for u in range(U):
        lo, hi = int(offsets[u]), int(offsets[u + 1])
        out = viterbi(c[lo:hi], lams[u])
        codes[lo:hi], dist[lo:hi], cost[u], n_seg[u] = out["codes"], out["dist"], out["cost"], out["n_seg"]
    return codes, dist, cost, n_seg, int((~np.isfinite(cost)).sum())


# ---- float64 yardsticks ------------------------------------------------------------------------------------------------------
def objective64(c, codes, lam):
    """sum of the chosen local costs + lam * changes, in float64 (lam = inf: inf unless there is no change)."""
    c = np.asarray(c, np.float64)
    codes = np.asarray(codes)
    changes = int((codes[1:] != codes[:-1]).sum())
    return c[np.arange(len(codes)), codes].sum() + (float(lam) * changes if changes else 0.0)


def brute_force64(c, lam):
    """The float64 minimum of the objective over all K^T labellings."""
    T, K = c.shape
    return min(objective64(c, np.array(lab), lam) for lab in itertools.product(range(K), repeat=T))


def viterbi64(c, lam):
    """The float64 optimum of the objective by the plain recurrence on running sums."""
    c = np.asarray(c, np.float64)
    r = c[0].copy()
    for t in range(1, len(c)):
        r = c[t] + np.minimum(r, r.min() + float(lam))
    return r.min()


# ---- the shapes both the host twin (CPU) and the kernels (GPU) are checked on ---------------------------------------------------
# k_seg_cost works on slabs of 64 frames x groups of 256 entries: the mixes below total 324 rows (five whole slabs and four
# rows) and 33 + 70 + 5 = 108 rows (one slab and 44 rows); K = 256 is one whole group, 257 one group and one entry, 4096 sixteen
# groups; K = 64 / 65 / 130 are the ballot-word edges of k_seg_scan (one word; one word and one bit; three words).
SLAB, GROUP = 64, 256
T_MIX = (1, 2, 0, 63, 64, 65, 129)                             # with an empty utterance between the others


def _lams(metric, n, rs):
    """A different penalty per utterance: 0, 1e30, inf and mid values at the scale of one frame's distance."""
    mid = 0.08 if metric == "scaled_l2" else 2.5
    base = [0.0, mid, 1e30, np.inf, mid / 4, 3 * mid, mid]
    return np.array([base[i % len(base)] for i in range(n)], F32)


def make_case(name, K, d, d_pitch, Ts, metric, seed, ties=False, nan_at=None):
    """dict(name, frames (n, d_pitch) fp32 with NaN in the pad channels, offsets, emb (K, d), metric, lams)."""
    rs = np.random.RandomState(seed)
    n = int(sum(Ts))
    if ties:                                                     # small integers: equal costs and equal r at a switch, exactly
        z = rs.randint(-2, 3, (n, d)).astype(F32)
        emb = rs.randint(-2, 3, (K, d)).astype(F32)
        emb[K // 2:] = emb[:K - K // 2]                          # every row twice
        lams = np.array([[0.0, 1.0, 2.0, 3.0, np.inf][i % 5] for i in range(len(Ts))], F32)
    else:
        z = rs.standard_normal((n, d)).astype(F32)
        emb = rs.standard_normal((K, d)).astype(F32)
        lams = _lams(metric, len(Ts), rs)
    frames = np.full((n, d_pitch), np.nan, F32)
    frames[:, :d] = z
    offsets = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64)
    if nan_at is not None:
        u, t = nan_at
        frames[offsets[u] + t, d // 2] = np.nan
    return dict(name=name, frames=frames, offsets=offsets, emb=emb, metric=metric, lams=lams, d=d)


def gpu_cases():
    cases = []
    for i, K in enumerate((1, 3, 64, 65, 130, 256, 257)):
        for metric in ("scaled_l2", "sq_l2"):
            cases.append(make_case(f"K{K}-{metric}", K, 8, 12, T_MIX, metric, 100 + i))
    for i, d in enumerate((1, 3, 32, 64, 65)):
        cases.append(make_case(f"d{d}", 130, d, d + 3, (33, 70, 0, 5), ("scaled_l2", "sq_l2")[i % 2], 200 + i))
    cases.append(make_case("d64-full", 70, 64, 68, (5, 70), "scaled_l2", 210))
    cases.append(make_case("K4096", 4096, 64, 64, (5,), "scaled_l2", 300))
    cases.append(make_case("ties-dup", 10, 3, 4, (40, 1, 66), "sq_l2", 400, ties=True))
    cases.append(make_case("ties-dup-130", 130, 2, 4, (70,), "sq_l2", 401, ties=True))
    cases.append(make_case("nan-mid", 65, 8, 8, (20, 33, 7), "scaled_l2", 500, nan_at=(1, 16)))
    cases.append(make_case("nan-mid-sq", 65, 8, 8, (20, 33, 7), "sq_l2", 501, nan_at=(1, 16)))
    return cases


_WANT = {}


def expected(case):
    """segment_ragged of a case, computed once per process and shared."""
    if case["name"] not in _WANT:
        d = case["d"]
        _WANT[case["name"]] = segment_ragged(np.ascontiguousarray(case["frames"][:, :d]), case["offsets"], case["emb"],
                                             case["metric"], case["lams"])
    return _WANT[case["name"]]
