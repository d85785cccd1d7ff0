"""TEST INFRASTRUCTURE - AEW_OP_GRAD_WELFORD and AEW_OP_SEG_SELECT restated in numpy (the arithmetic of aew_grad_welford_t
/ aew_seg_select_t, include/aewavenet.h): fp32 round-to-nearest element updates, fp64 chunk sums in the documented order,
and a sort-based selection under the op's order key.  The device is held to it bit for bit.  Not part of the product."""
import numpy as np

F = np.float32
CHUNK = 4096
NAN_KEY = np.uint32(0xFFFFFFFF)


def welford(g, mu, s, first, divisor):
    """One sample folded in: (mu', s').  first: mu = g, s = 0 (mu / s are not read)."""
    g = np.asarray(g, F)
    if first:
        return g.copy(), np.zeros_like(g)
    with np.errstate(all="ignore"):
        d = g - mu
        mu2 = mu + d / F(divisor)
        return mu2, s + d * (g - mu2)


def select_key(x):
    """uint32 order key: the bit pattern for x >= 0 (-0 as +0), 0xFFFFFFFF for x < 0 or NaN."""
    x = np.ascontiguousarray(x, F)
    with np.errstate(invalid="ignore"):
        return np.where(x >= 0, x.view(np.uint32) & np.uint32(0x7FFFFFFF), NAN_KEY).astype(np.uint32)


def kth(x, k, raw=True, denom=1.0):
    """out of the op for one tensor and one 1-based rank."""
    x = np.asarray(x, F).reshape(-1)
    if x.size == 0 or not 1 <= k <= x.size:
        return F(np.nan)
    key = np.sort(select_key(x), kind="stable")[k - 1]
    if key == NAN_KEY:
        return F(np.nan)
    v = np.array([key], np.uint32).view(F)[0]
    if raw:
        return v
    with np.errstate(all="ignore"):
        return np.sqrt(v / F(denom))


def seg_select(s, offs, lens, ks, raw=True, denom=1.0):
    """[P][Q] float32: kth() of every tensor s[offs[t] : offs[t] + lens[t]] for the ranks ks[t]."""
    out = np.full((len(offs), len(ks[0])), np.nan, F)
    for t, (o, n) in enumerate(zip(offs, lens)):
        for q, k in enumerate(ks[t]):
            out[t, q] = kth(s[o:o + n], int(k), raw, denom)
    return out


def same_numbers(a, b):
    """NaN matches NaN, +0 equals -0, bits are identical otherwise."""
    a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    zero = (a == 0) & (b == 0)
    return bool(np.all(nan | zero | (a.view(np.uint32) == b.view(np.uint32))))


def ranks(qs, numel):
    """grad_analysis.py:48 - Python's round (half to even), 1-based."""
    return [1 + round(float(q) * (numel - 1)) for q in qs]


# ---- the fp64 sums: per thread one chain, butterfly inside the wave, waves ascending (gn_block_sum)
def block_sum(v):
    """v: float64 [256] per-thread values -> the block's total."""
    v = np.asarray(v, np.float64).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        v = v + v[:, lane ^ o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def chunk_sum(x):
    """Sum of the float64 values x (one chunk, <= CHUNK of them): thread t chains elements (it * 256 + t) * 4 + r, it and r
    ascending.  (An absent element adds nothing; adding +0.0 instead is the same in every bit.)"""
    buf = np.zeros(CHUNK, np.float64)
    buf[:len(x)] = x
    buf = buf.reshape(CHUNK // 1024, 256, 4)
    acc = np.zeros(256, np.float64)
    for it in range(CHUNK // 1024):
        for r in range(4):
            acc = acc + buf[it, :, r]
    return block_sum(acc)


def chunk_table(offs, lens):
    """[(off, len, tensor)] and first[P + 1]: aew_uw_chunks by hand."""
    chunks, first = [], []
    for t, (o, n) in enumerate(zip(offs, lens)):
        first.append(len(chunks))
        for c in range(0, n, CHUNK):
            chunks.append((o + c, min(CHUNK, n - c), t))
    return chunks, first + [len(chunks)]


def part_sums(mu, s, offs, lens):
    """part[n_chunks][2] = {sum s, sum mu^2} per chunk."""
    chunks, _ = chunk_table(offs, lens)
    part = np.zeros((len(chunks), 2), np.float64)
    for c, (o, n, _) in enumerate(chunks):
        m = mu[o:o + n].astype(np.float64)
        part[c] = chunk_sum(s[o:o + n].astype(np.float64)), chunk_sum(m * m)
    return part


def tensor_sums(part, first):
    """AEW_OP_UPDATE_RATIO with finalize = 0: [2][P]; thread t adds the run [t * per, (t + 1) * per) of the tensor's chunks."""
    P = len(first) - 1
    out = np.zeros((2, P), np.float64)
    for t in range(P):
        c0, nc = first[t], first[t + 1] - first[t]
        per = (nc + 255) // 256
        for j in range(2):
            acc = np.zeros(256, np.float64)
            for th in range(256):
                q0 = min(nc, th * per)
                for q in range(q0, min(nc, q0 + per)):
                    acc[th] = acc[th] + part[c0 + q, j]
            out[j, t] = block_sum(acc)
    return out


def padded_offsets(lens):
    """The ParamStore rule: every tensor starts at a multiple of 4."""
    offs, o = [], 0
    for n in lens:
        offs.append(o)
        o += (n + 3) // 4 * 4
    return offs, o
