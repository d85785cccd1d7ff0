"""TEST INFRASTRUCTURE - plain float64 definitions of the training step's non-GEMM ops.

One numpy function per op, written from the formulas in include/aewavenet.h and the reference model lines the kernel
comments cite - not from the kernel loops and not from tests/plan_emulator.py (nothing is imported from it).  Inputs are
plain arrays and integers, results are plain float64 arrays (bf16 / fp32 *storage* results, which are exact to restate,
are float32 arrays that hold the stored value).  Every function is linear or monotone enough in its inputs that calling
it on the absolute values of the inputs yields the sum of the absolute values of the terms an output element adds up;
the tests use that for their error bounds.
"""
import numpy as np


# ---- storage helpers ----------------------------------------------------------------------------
def f32(x):
    """x rounded to float32 (round to nearest even, numpy's conversion)."""
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def rne_bf16(x_fp32):
    """float32 -> bfloat16 by round-to-nearest-even on the bit pattern; returned as the float32 that holds the bf16
    value (low 16 bits zero).  Finite inputs only."""
    b = np.ascontiguousarray(np.asarray(x_fp32, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x_fp32))


def pack_index(co, gate):
    """Packed channel of the gated layers: n = (co >> 4) * 32 + (co & 15) + 16 * gate (filter 0, gate 1)."""
    co = np.asarray(co)
    return (co >> 4) * 32 + (co & 15) + 16 * gate


# ---- softmax + NLL  (wavenet.py:543-547) --------------------------------------------------------
def _targets(wav, tgt_off, w):
    """target of position u is wav[tgt_off + u + 1]; the last position w - 1 has none (returned as class 0, not live)."""
    wav = np.asarray(wav)
    tgt = np.zeros((wav.shape[0], w), dtype=np.int64)
    tgt[:, :w - 1] = wav[:, tgt_off + 1: tgt_off + w].astype(np.int64)
    live = np.ones((wav.shape[0], w), dtype=bool)
    live[:, w - 1] = False
    return tgt, live


def softmax_parts(logits):
    """(max, sum exp(l - max), log-softmax) of the last axis, float64."""
    lg = np.asarray(logits, dtype=np.float64)
    mx = lg.max(-1)
    se = np.exp(lg - mx[..., None]).sum(-1)
    return mx, se, lg - (mx + np.log(se))[..., None]


def softmax_nll_fwd(logits, wav, tgt_off):
    """logits [B][w][Q] -> (nll, ptgt, peak, amax), each [B][w].
    Rules: the target of position u is wav[b][tgt_off + u + 1]; position w - 1 carries no loss: nll = ptgt = 0 there.
    peak = max_c log p(c) is defined for EVERY position, amax is the LOWEST class that holds the maximum."""
    B, w, Q = np.shape(logits)
    tgt, live = _targets(wav, tgt_off, w)
    mx, se, lsm = softmax_parts(logits)
    lp = np.take_along_axis(lsm, tgt[..., None], -1)[..., 0]
    nll = np.where(live, -lp, 0.0)
    ptgt = np.where(live, np.exp(lp), 0.0)
    return nll, ptgt, -np.log(se), np.argmax(np.asarray(logits, dtype=np.float64), -1).astype(np.int32)


def softmax_nll_bwd(logits, wav, tgt_off, scale, Q_pad, gmul=None):
    """d(scale * gmul * sum nll)/d(logits) -> [B][w][Q_pad] float64 (before the bf16 storage rounding).
    Rules: scale is multiplied by gmul[0] when gmul is present; the row of position w - 1 is zero; columns Q..Q_pad are
    zero."""
    B, w, Q = np.shape(logits)
    tgt, live = _targets(wav, tgt_off, w)
    _, _, lsm = softmax_parts(logits)
    sc = float(scale) * (1.0 if gmul is None else float(gmul))
    g = np.exp(lsm)
    np.put_along_axis(g, tgt[..., None], np.take_along_axis(g, tgt[..., None], -1) - 1.0, -1)
    out = np.zeros((B, w, Q_pad))
    out[:, :, :Q] = np.where(live[..., None], g * sc, 0.0)
    return out


# ---- base layer: one-hot x 1x1 conv == column gather  (wavenet.py:348-351) ----------------------
def base_gather(wav, wav_off, T, W, bias, R_pad, ones_channel, Q_pad=None):
    """x[b][t][c] = rne_bf16(f32(W[c][q]) + f32(bias[c])), q = wav[b][wav_off + t]: ONE fp32 add, exact to restate.
    Rules: no bias -> rne_bf16(W[c][q]); the ones channel is column R (when asked for, R < R_pad); every other pad column
    is zero; the one-hot [B][T][Q_pad] is exactly 1.0 at q and 0 elsewhere.  Returns (x, onehot or None) as float32."""
    wav = np.asarray(wav)
    W = np.asarray(W, dtype=np.float32)
    R, Q = W.shape
    q = wav[:, wav_off: wav_off + T].astype(np.int64)
    v = W.T[q]                                                   # [B][T][R]
    if bias is not None:
        v = (v + np.asarray(bias, dtype=np.float32)[None, None, :]).astype(np.float32)
    x = np.zeros(q.shape + (R_pad,), dtype=np.float32)
    x[..., :R] = rne_bf16(v)
    if ones_channel:
        x[..., R] = 1.0
    oh = None
    if Q_pad is not None:
        oh = np.zeros(q.shape + (Q_pad,), dtype=np.float32)
        np.put_along_axis(oh, q[..., None], 1.0, -1)
    return x, oh


# ---- jitter gather / scatter  (wavenet.py:330-336) ----------------------------------------------
def _lc_source_index(jitter, B, N, C, take_compat):
    """Flat index into the [B][N][C] source for every output element (b, t, c).
    Rules: jitter indices are clamped to [0, N - 1].  take_compat = 0: (b, j, c).  take_compat = 1 (SURVEY C-1): the
    reference calls torch.take on the (B, C, N) tensor with index b * N + j, the same for every channel c: the flat
    element b * N + j of the NCL layout, i.e. (b', c', n') = (flat // (C N), (flat // N) % C, flat % N)."""
    j = np.clip(np.asarray(jitter)[:B, :N].astype(np.int64), 0, N - 1)
    b = np.arange(B)[:, None, None]
    c = np.arange(C)[None, None, :]
    if not take_compat:
        return (b * N + j[:, :, None]) * C + c
    flat = np.broadcast_to((b * N + j[:, :, None]), (B, N, C))   # index into the flattened (B, C, N) tensor
    bb, cc, nn = flat // (C * N), (flat // N) % C, flat % N
    return (bb * N + nn) * C + cc


def lc_gather(src, jitter, C_pad, take_compat):
    """src [B][N][C] fp32 -> rne_bf16 of the gathered rows, [B][N][C_pad] float32; pad columns are zero."""
    src = np.asarray(src, dtype=np.float32)
    B, N, C = src.shape
    out = np.zeros((B, N, C_pad), dtype=np.float32)
    out[:, :, :C] = rne_bf16(src.reshape(-1)[_lc_source_index(jitter, B, N, C, take_compat)])
    return out


def lc_gather_f64(src, jitter, take_compat):
    """The gather without storage rounding (for the adjoint identity)."""
    src = np.asarray(src, dtype=np.float64)
    B, N, C = src.shape
    return src.reshape(-1)[_lc_source_index(jitter, B, N, C, take_compat)]


def lc_scatter(d, jitter, take_compat):
    """The exact adjoint of the gather: dsrc[source element] = sum of d over the output elements that read it.
    [B][N][C] -> [B][N][C] float64; source elements nobody read are zero."""
    d = np.asarray(d, dtype=np.float64)
    B, N, C = d.shape
    out = np.zeros(B * N * C)
    np.add.at(out, _lc_source_index(jitter, B, N, C, take_compat).reshape(-1), d.reshape(-1))
    return out.reshape(B, N, C)


# ---- speaker-conditioned gated bias  (wavenet.py:135-139 folded) --------------------------------
def spk_gc(params, voice, off_spk_w, off_spk_b, G, n_speakers):
    """gc[b][j] = Wspk[j][voice[b]] (+ bspk[j] unless off_spk_b == -1)."""
    p = np.asarray(params, dtype=np.float64)
    Wsp = p[off_spk_w: off_spk_w + G * n_speakers].reshape(G, n_speakers)
    gc = Wsp[:, np.asarray(voice, dtype=np.int64)].T.copy()
    if off_spk_b >= 0:
        gc += p[off_spk_b: off_spk_b + G][None, :]
    return gc


def spk_bias(params, voice, off_bias, off_proj, off_spk_w, off_spk_b, L, D, D_pad, C_lc, G, n_speakers):
    """bias[b][l][pack(co, gate)] = conv_bias_l,gate[co] + sum_j V_l,gate[co][C_lc + j] * gc[b][j]  -> ([B][L][2 D_pad], gc).
    off_bias / off_proj: [2][L] offsets into params (filter row 0, gate row 1); V is [D][C_lc + G] row-major.
    Rules: packed channel n = (co >> 4) * 32 + (co & 15) + 16 * gate; a layer whose bias offset is -1 has no bias term;
    off_spk_b == -1 is allowed (no embedding bias); packed channels of co >= D are zero."""
    p = np.asarray(params, dtype=np.float64)
    gc = spk_gc(params, voice, off_spk_w, off_spk_b, G, n_speakers)
    out = np.zeros((len(voice), L, 2 * D_pad))
    co = np.arange(D)
    for l in range(L):
        for gate in (0, 1):
            ov, ob = int(off_proj[gate][l]), int(off_bias[gate][l])
            V = p[ov: ov + D * (C_lc + G)].reshape(D, C_lc + G)[:, C_lc:]
            v = gc @ V.T
            if ob >= 0:
                v = v + p[ob: ob + D][None, :]
            out[:, l, pack_index(co, gate)] = v
    return out, gc


def spk_colsum_per_element(colsum, colsum_running):
    """colsum [B][L][2 D_pad]; the first `colsum_running` layers hold running sums over batch elements 0..b: their
    per-element value is colsum[b] - colsum[b - 1] (b = 0: colsum[0])."""
    cs = np.array(colsum, dtype=np.float64)
    r = min(int(colsum_running), cs.shape[1])
    if r > 0:
        cs[1:, :r] = cs[1:, :r] - np.asarray(colsum, dtype=np.float64)[:-1, :r]
    return cs


def spk_bwd(params, voice, off_bias, off_proj, off_spk_w, off_spk_b, L, D, D_pad, C_lc, G, n_speakers,
            cs, gc, grads_in, first=0, count=None):
    """Gradient of <spk_bias(params), cs> with cs the PER-ELEMENT column sums (spk_colsum_per_element) -> grads (flat).
    Rules: the op covers layers [first, first + count) (count None: all); it OVERWRITES the bias and projection
    (columns C_lc..C_lc+G of V) gradients of those layers only - a bias offset of -1: no bias gradient - and ADDS the
    speaker-embedding sums (and the embedding-bias sums unless off_spk_b == -1) into grads.  Everything else in grads,
    the rows of speakers absent from `voice` included, is untouched."""
    p = np.asarray(params, dtype=np.float64)
    g = np.array(grads_in, dtype=np.float64)
    cs = np.asarray(cs, dtype=np.float64)
    gc = np.asarray(gc, dtype=np.float64)
    B = len(voice)
    co = np.arange(D)
    dgc = np.zeros((B, G))
    for l in range(first, first + (L if count is None else count)):
        for gate in (0, 1):
            ov, ob = int(off_proj[gate][l]), int(off_bias[gate][l])
            c = cs[:, l, pack_index(co, gate)]                    # [B][D]
            if ob >= 0:
                g[ob: ob + D] = c.sum(0)
            gv = g[ov: ov + D * (C_lc + G)].reshape(D, C_lc + G)  # a view: written in place
            gv[:, C_lc:] = c.T @ gc
            dgc += c @ p[ov: ov + D * (C_lc + G)].reshape(D, C_lc + G)[:, C_lc:]
    gw = g[off_spk_w: off_spk_w + G * n_speakers].reshape(G, n_speakers)
    for b in range(B):
        gw[:, int(voice[b])] += dgc[b]
    if off_spk_b >= 0:
        g[off_spk_b: off_spk_b + G] += dgc.sum(0)
    return g


# ---- VQ backward  (vqema_bn.py:44-45, vq_bn.py:78) ----------------------------------------------
def vq_dist(z, c, metric):
    """metric 0 (scaled_l2): ||z - c|| / (||z|| + ||c||); metric 1 (sq_l2): ||z - c||^2.  Per row."""
    t = z - c
    if metric == 0:
        return np.sqrt((t * t).sum(-1)) / (np.sqrt((z * z).sum(-1)) + np.sqrt((c * c).sum(-1)))
    return (t * t).sum(-1)


def vq_bwd_terms(ze, emb, ind, metric):
    """The two terms of d(dist)/d(z) for each query [Q][d] (their sum is the gradient).
    metric 0: u = ||z - c||, v = ||z|| + ||c||:  t1 = (z - c) / (u v),  t2 = -u z / (v^2 ||z||).
    Rules: t1 = 0 where u == 0 (z equals its code), t2 = 0 where ||z|| == 0.   metric 1: t1 = 2 (z - c), t2 = 0."""
    z = np.asarray(ze, dtype=np.float64)
    c = np.asarray(emb, dtype=np.float64)[np.asarray(ind, dtype=np.int64)]
    t = z - c
    if metric != 0:
        return 2.0 * t, np.zeros_like(t)
    u = np.sqrt((t * t).sum(-1, keepdims=True))
    zn = np.sqrt((z * z).sum(-1, keepdims=True))
    v = zn + np.sqrt((c * c).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = np.where(u > 0, t / (u * v), 0.0)
        t2 = np.where(zn > 0, -u * z / (v * v * zn), 0.0)
    return t1, t2


def vq_bwd(ze, emb, ind, dzq, metric, coef, demb_coef=0.0, gmul=None, demb_in=None):
    """dze = dzq (straight through) + coef * gmul * d(dist)/d(z);  demb (when demb_in is given) = demb_in + for each code
    the sum over the queries that chose it of demb_coef * gmul * (-2) (z - c).  Rows of codes nobody chose are not
    touched.  -> (dze [Q][d], demb [K][d] or None)."""
    gm = 1.0 if gmul is None else float(gmul)
    t1, t2 = vq_bwd_terms(ze, emb, ind, metric)
    dze = np.asarray(dzq, dtype=np.float64) + float(coef) * gm * (t1 + t2)
    demb = None
    if demb_in is not None:
        demb = np.array(demb_in, dtype=np.float64)
        t = np.asarray(ze, dtype=np.float64) - np.asarray(emb, dtype=np.float64)[np.asarray(ind, dtype=np.int64)]
        np.add.at(demb, np.asarray(ind, dtype=np.int64), float(demb_coef) * gm * (-2.0) * t)
    return dze, demb


# ---- VAE  (vae_bn.py:44-53, 90-98) --------------------------------------------------------------
def vae_fwd(mu, ls, eps):
    """sample = mu + exp(ls / 2) * eps [Q][d];  kl_terms[q] = sum_j (1 + ls - mu^2 - exp(ls))."""
    mu, ls, eps = (np.asarray(a, dtype=np.float64) for a in (mu, ls, eps))
    return mu + np.exp(0.5 * ls) * eps, (1.0 + ls - mu * mu - np.exp(ls)).sum(-1)


def vae_bwd(mu, ls, eps, dsample, kl_coef, gmul=None, kl_value=None, free_nats=0.0):
    """Gradient of <sample, dsample> + k * KL, KL = -0.5 sum (1 + ls - mu^2 - exp(ls)), with respect to (mu, ls).
    Rules: k = kl_coef (host or device value - the caller passes whichever applies) times gmul when present; when
    kl_value is given the KL part is gated by [kl_value >= free_nats] (the backward of torch.clamp(kl, min=free_nats))."""
    mu, ls, eps, ds = (np.asarray(a, dtype=np.float64) for a in (mu, ls, eps, dsample))
    k = float(kl_coef) * (1.0 if gmul is None else float(gmul))
    if kl_value is not None and not (float(kl_value) >= float(free_nats)):
        k = 0.0
    return ds + k * mu, ds * eps * 0.5 * np.exp(0.5 * ls) + k * (-0.5) * (1.0 - np.exp(ls))


# ---- AE norm term  (ae_bn.py:36-38) -------------------------------------------------------------
def ae_norm_fwd(ze):
    """term[q] = | ||ze[q]|| - 1 |."""
    z = np.asarray(ze, dtype=np.float64)
    return np.abs(np.sqrt((z * z).sum(-1)) - 1.0)


def ae_norm_bwd(ze, dze_in, coef, gmul=None):
    """dze = dze_in + coef * gmul * sgn(||z|| - 1) * z / ||z||.  Rules: sgn = 0 at norm exactly 1; the term is 0 at norm 0."""
    z = np.asarray(ze, dtype=np.float64)
    nrm = np.sqrt((z * z).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(nrm > 0, np.sign(nrm - 1.0) * z / nrm, 0.0)
    return np.asarray(dze_in, dtype=np.float64) + float(coef) * (1.0 if gmul is None else float(gmul)) * term
