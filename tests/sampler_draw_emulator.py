"""Numpy restatement of the sampler's draw controls (include/aewavenet.h: aew_draw_t; ae_wavenet_amd/sampler.py: Draw,
draw_table; csrc/aew_sampler.hip: the DRAW instantiation): the order, the K-set, the P-set and the inverse-CDF draw over
what is kept, one stream and one step at a time.  The weight ARGUMENT is the fp32 product the kernel forms, (l - max l) *
inv_temp; everything after it is float64, so a decision the kernel takes in fp32 can differ from the one here only where
it hangs on less than the fp32 summation error - and `ambiguous` says where that is.  Written from the header's text and
the issue; shares no code with the package."""
import numpy as np

EPS_REL = 1e-5                       # fp32 summation order, as a share of the total (tests/test_sampler.py, check (d))
NEUTRAL = (1.0, 0, 1.0, False)


def order(l):
    """Indices of l, first to last: l[i] > l[j], or l[i] == l[j] and i < j (-0 == +0, as the comparison has it)."""
    l = np.asarray(l, np.float32) + np.float32(0.0)
    return np.lexsort((np.arange(l.size), -l.astype(np.float64)))       # (stable keys: value down, then index up)


def key_bits(l):
    """The order-preserving 32-bit key of fp32 logits: key[i] > key[j] <=> l[i] > l[j] (-0 folded into +0)."""
    b = (np.asarray(l, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def k_set(l, top_k):
    """Boolean mask of the K-set: the first top_k values in the order; <= 0 or >= Q means all.  Logit bits only."""
    Q = len(l)
    keep = np.zeros(Q, bool)
    keep[order(l)[:Q if (top_k <= 0 or top_k >= Q) else top_k]] = True
    return keep


def weights(l, inv_temp):
    """float64 exp of the fp32 argument (l - max l) * inv_temp."""
    l = np.asarray(l, np.float32)
    arg = (l - l.max()) * np.float32(inv_temp)                           # fp32 subtraction, fp32 product
    assert arg.dtype == np.float32
    return np.exp(arg.astype(np.float64))


def draw(l, u, inv_temp=1.0, top_k=0, top_p=1.0, greedy=False):
    """(value, kept mask, ambiguous) for logits l[Q] and the uniform u.  ambiguous: the weight mass preceding some value of
    the K-set lies within EPS_REL * (K-set sum) of the nucleus target, so the P-set is not decided at fp32 accuracy."""
    l = np.asarray(l, np.float32)
    Q = l.size
    o = order(l)
    if greedy:
        keep = np.zeros(Q, bool)
        keep[o[0]] = True
        return int(o[0]), keep, False
    w = weights(l, inv_temp)
    keep = k_set(l, top_k)
    ambiguous = False
    if top_p <= 0:
        keep = np.zeros(Q, bool)
        keep[o[0]] = True
    elif top_p < 1:
        ko = o[keep[o]]                                                  # the K-set in the order
        total = w[ko].sum()
        target = float(np.float32(top_p)) * total
        before = np.concatenate([[0.0], np.cumsum(w[ko])[:-1]])         # mass preceding each value
        inside = before < target                                         # shortest prefix whose sum reaches the target
        inside[0] = True
        ambiguous = bool((np.abs(before[1:] - target) <= EPS_REL * total).any())
        keep = np.zeros(Q, bool)
        keep[ko[inside]] = True
    wk = np.where(keep, w, 0.0)
    cum = np.cumsum(wk)                                                  # index order
    hit = np.nonzero(cum > float(np.float32(u)) * cum[-1])[0]
    value = int(hit[0]) if hit.size else int(np.nonzero(keep)[0][-1])
    return value, keep, ambiguous


def interval_ok(l, u, value, keep, inv_temp=1.0):
    """Check (d) of tests/test_sampler.py over a kept set: `value` is kept and u * total lies in the cumulative interval
    of `value`, within EPS_REL * total."""
    wk = np.where(keep, weights(l, inv_temp), 0.0)
    cum = np.cumsum(wk)
    target = float(np.float32(u)) * cum[-1]
    lo = cum[value - 1] if value else 0.0
    eps = EPS_REL * cum[-1]
    return bool(keep[value]) and lo - eps <= target <= cum[value] + eps
