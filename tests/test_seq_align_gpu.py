"""AEW_OP_SEQ_ALIGN on the device: the op alone, bit for bit against its numpy restatement (tests/seq_align_emulator.py)
with canaries around every output and outputs at odd element offsets - every strip and tile edge of a 64-wide design,
every register instantiation of D, both layouts, ties, EDIT with symbols that are no index, empty and non-finite pairs,
paths, the split under max_back_bytes, refused records - then the surface (align.py, model.code_distance /
cepstral_distance, codes.mu_decode) and one plan replayed from a captured graph."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL, codes as CD
from ae_wavenet_amd.plan import Plan
from tests import seq_align_emulator as SE
from tests.test_codes_gpu import _bits, _model
from tests.test_utterance_gpu import _engine_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CAN = 65                                                     # canary elements in front of and behind every output (odd: the
LENS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 257)        # outputs then start at odd element offsets)
SMALL = (1, 63, 65, 129)
METRIC = {"euclid": SE.EUCLID, "sqeuclid": SE.SQEUCLID}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- data sets and their emulator results, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seqs(kind, D, lens):
    rs = np.random.RandomState(D * 1000 + len(lens) + (7 if kind == "binary" else 0))
    draw = (lambda n: rs.randint(0, 2, (n, D)).astype(F32)) if kind == "binary" else (lambda n: rs.randn(n, D).astype(F32))
    return [draw(n) for n in lens], [draw(n) for n in lens]


def _all_pairs(k):
    return [(a, b) for a in range(k) for b in range(k)]


@functools.lru_cache(maxsize=None)
def _want(kind, D, lens, metric):
    A, B = _seqs(kind, D, lens)
    return [SE.dtw(A[a], B[b], METRIC[metric], want_back=True) for a, b in _all_pairs(len(lens))]


# ---- one launch of the op on raw buffers ---------------------------------------------------------------------------------
class _Side:
    """Sequences laid out in one buffer: frame-major rows, or channel-major (D, n) arrays (element (i, k) at
    base + i + k * n) - the same values."""

    def __init__(self, seqs, layout, dtype=np.float32):
        D = seqs[0].shape[1] if seqs[0].ndim == 2 else 1
        t = np.zeros(len(seqs), dtype=L.ALIGN_SEQ_DTYPE)
        parts, at = [], 3                                    # (a few elements in front: bases are not 0)
        for u, s in enumerate(seqs):
            n = s.shape[0]
            t["base"][u], t["len"][u] = at, n
            t["frame_stride"][u], t["chan_stride"][u] = (D, 1) if layout == "frame" else (1, n)
            parts.append(np.ascontiguousarray(s if layout == "frame" else s.reshape(n, D).T).reshape(-1))
            at += n * D
        self.host = t
        self.flat = _dev(np.concatenate([np.full(3, 77, dtype)] + [p.astype(dtype) for p in parts] + [np.full(5, 77, dtype)]))
        self.table = _dev(t.view(np.uint8).reshape(-1).copy())
        self.lens, self.D = [s.shape[0] for s in seqs], D


def _canaried(n, dtype, fill):
    buf = torch.full((n + 2 * CAN,), fill, dtype=dtype, device=DEV)
    return buf, buf[CAN:CAN + n]


def _intact(buf, n, fill):
    return bool((buf[:CAN] == fill).all()) and bool((buf[CAN + n:] == fill).all())


class _Launch:
    def __init__(self, mode, metric, sa, sb, pairs, back=False, path=False, ws=True):
        self.sa, self.sb, self.pairs = sa, sb, pairs
        pr = np.asarray(pairs, np.int64)
        tp, chunks, n_back, n_path, wstride = AL.pair_table(sa.lens, sb.lens, pr, None)
        self.tp, self.P, self.n_back, self.n_path = tp, len(pairs), n_back, n_path
        self.d_tp = _dev(tp.view(np.uint8).reshape(-1).copy())
        self.cost_buf, self.cost = _canaried(self.P, torch.float32, -7.0)
        self.steps_buf, self.steps = _canaried(self.P, torch.int32, -7)
        self.bad = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.back_buf, self.back = _canaried(max(n_back, 1), torch.uint8, 9) if back else (None, None)
        self.path_buf, self.path = _canaried(2 * max(n_path, 1), torch.int32, -7) if path else (None, None)
        self.ws = torch.empty(max(2 * self.P * wstride[0], 1), dtype=torch.float32, device=DEV) if ws and wstride[0] else None
        r = self.rec = L.SeqAlign()
        r.mode, r.metric, r.D, r.n_pairs = mode, metric, sa.D, self.P
        r.seq_a, r.seq_a_host, r.n_a = sa.table.data_ptr(), sa.host.ctypes.data, len(sa.host)
        r.seq_b, r.seq_b_host, r.n_b = sb.table.data_ptr(), sb.host.ctypes.data, len(sb.host)
        r.pairs, r.pairs_host = self.d_tp.data_ptr(), tp.ctypes.data
        r.feat_a, r.n_feat_a, r.feat_b, r.n_feat_b = sa.flat.data_ptr(), sa.flat.numel(), sb.flat.data_ptr(), sb.flat.numel()
        r.cost, r.steps, r.bad = self.cost.data_ptr(), self.steps.data_ptr(), self.bad.data_ptr()
        if self.ws is not None:
            r.ws, r.ws_bytes = self.ws.data_ptr(), 4 * self.ws.numel()
        if back:
            r.back, r.n_back = self.back.data_ptr(), n_back
        if path:
            r.path, r.n_path = self.path.data_ptr(), n_path

    def run(self):
        CD._run(L.OP_SEQ_ALIGN, self.rec, "seq align", torch.device(DEV))
        return self

    def rc(self):
        op = L.Op()
        op.kind, op.u.align = L.OP_SEQ_ALIGN, self.rec
        st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        return L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(st), None)

    def untouched(self):
        torch.cuda.synchronize()
        ok = bool((self.cost_buf == -7.0).all()) and bool((self.steps_buf == -7).all()) and not bool(self.bad.any())
        if self.back_buf is not None:
            ok = ok and bool((self.back_buf == 9).all())
        if self.path_buf is not None:
            ok = ok and bool((self.path_buf == -7).all())
        return ok

    def results(self):
        """(cost bytes per pair, steps, bad) after the canary checks."""
        torch.cuda.synchronize()
        assert _intact(self.cost_buf, self.P, -7.0) and _intact(self.steps_buf, self.P, -7), "canaries around cost / steps"
        assert not self.bad[1:].any()
        if self.back_buf is not None:
            assert _intact(self.back_buf, max(self.n_back, 1), 9), "canaries around back"
        if self.path_buf is not None:
            assert _intact(self.path_buf, 2 * max(self.n_path, 1), -7), "canaries around path"
        self.back_np = self.back.cpu().numpy() if self.back is not None else None
        self.path_np = self.path.cpu().numpy() if self.path is not None else None
        return self.cost.cpu().numpy(), self.steps.cpu().numpy(), int(self.bad[0].item()) & 0xFFFFFFFF

    def back_of(self, p):
        a, b = self.pairs[p]
        n, m = self.sa.lens[a], self.sb.lens[b]
        lo = int(self.tp["back_base"][p])
        return self.back_np[lo:lo + n * m].reshape(n, m)

    def path_of(self, p):
        a, b = self.pairs[p]
        n, m = self.sa.lens[a], self.sb.lens[b]
        lo = 2 * int(self.tp["path_base"][p])
        return self.path_np[lo:lo + 2 * (n + m - 1)].reshape(n + m - 1, 2)


def _check_against(want, cost, steps):
    wc = np.array([w[0] for w in want], F32)
    ws = np.array([w[1] for w in want], np.int32)
    assert steps.tolist() == ws.tolist()
    assert cost.tobytes() == wc.tobytes()


# ---- DTW -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("kind,D", [("normal", 5), ("binary", 3)])
def test_dtw_equals_the_emulator_on_every_strip_and_tile_edge(kind, D, metric):
    """All 121 ordered pairs of LENS in one launch, with back-pointers and paths; the channel-major view of the same
    values; the same pairs without back-pointers.  The binary features put ties in most cells."""
    A, B = _seqs(kind, D, LENS)
    want = _want(kind, D, LENS, metric)
    pairs = _all_pairs(len(LENS))
    mt = METRIC[metric]
    first = _Launch(L.ALIGN_DTW, mt, _Side(A, "frame"), _Side(B, "frame"), pairs, back=True, path=True).run()
    cost, steps, bad = first.results()
    assert bad == 0
    _check_against(want, cost, steps)
    if kind == "binary":
        assert len({(w[1]) for w in want}) > 20                                   # (the tie order decides the path length)
    for p in range(len(pairs)):
        assert first.back_of(p).tobytes() == want[p][2].tobytes(), pairs[p]
        assert first.path_of(p).tobytes() == SE.walk(want[p][2], want[p][1]).tobytes(), pairs[p]
    other = _Launch(L.ALIGN_DTW, mt, _Side(A, "chan"), _Side(B, "chan"), pairs).run()     # channel-major, no back
    c2, s2, bad2 = other.results()
    assert bad2 == 0 and c2.tobytes() == cost.tobytes() and s2.tolist() == steps.tolist()
    mixed = _Launch(L.ALIGN_DTW, mt, _Side(A, "chan"), _Side(B, "frame"), pairs, back=True).run()
    c3, s3, _ = mixed.results()
    assert c3.tobytes() == cost.tobytes() and s3.tolist() == steps.tolist()
    assert mixed.back.cpu().numpy().tobytes() == first.back.cpu().numpy().tobytes()


@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("D", [1, 12, 13, 64, 65, 130])
def test_dtw_equals_the_emulator_for_every_way_D_is_held(D, metric):
    A, B = _seqs("normal", D, SMALL)
    want = _want("normal", D, SMALL, metric)
    pairs = _all_pairs(len(SMALL))
    outs = []
    for layout in ("frame", "chan"):
        run = _Launch(L.ALIGN_DTW, METRIC[metric], _Side(A, layout), _Side(B, layout), pairs, back=True, path=True).run()
        cost, steps, bad = run.results()
        assert bad == 0
        _check_against(want, cost, steps)
        outs.append((run.back.cpu().numpy().tobytes(), run.path.cpu().numpy().tobytes()))
        for p in (3, 7, 15):
            assert run.path_of(p).tobytes() == SE.walk(want[p][2], want[p][1]).tobytes()
    assert outs[0] == outs[1]


def test_one_by_many_and_many_by_one():
    A, B = _seqs("normal", 5, LENS)
    want = _want("normal", 5, LENS, "euclid")
    k = len(LENS)
    for p in (0 * k + k - 1, (k - 1) * k + 0):                                     # 1 x 257 and 257 x 1
        n, m = len(A[p // k]), len(B[p % k])
        assert want[p][1] == max(n, m) and (n, m) in ((1, 257), (257, 1))


# ---- EDIT ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", [2, 1000])
def test_edit_equals_the_emulator(alphabet):
    lens = (0,) + LENS
    rs = np.random.RandomState(alphabet)
    def draw(n):
        s = rs.randint(0, alphabet, n).astype(np.int64)
        if alphabet == 2:
            return np.where(s == 0, -1, 1 << 40).astype(np.int64)                    # compared, never used as an index
        return s // 2 + (s % 2) * (1 << 40)                                          # pairs of symbols equal in their low 32 bits
    A, B = [draw(n) for n in lens], [draw(n) for n in lens]
    B[5] = A[5].copy()                                                              # one equal pair
    pairs = _all_pairs(len(lens))
    run = _Launch(L.ALIGN_EDIT, 0, _Side(A, "frame", np.int64), _Side(B, "frame", np.int64), pairs).run()
    cost, steps, bad = run.results()
    want = [SE.edit(A[a], B[b]) for a, b in pairs]
    assert bad == 0 and steps.tolist() == want and cost.tolist() == [float(w) for w in want]
    assert want[5 * len(lens) + 5] == 0 and want[0] == 0 and want[1] == 1 and want[len(lens)] == 1


# ---- special pairs -------------------------------------------------------------------------------------------------------
def test_empty_and_non_finite_pairs():
    rs = np.random.RandomState(3)
    lens = (0, 5, 70, 0, 66)
    A = [rs.randn(n, 4).astype(F32) for n in lens]
    B = [rs.randn(n, 4).astype(F32) for n in lens]
    pairs = _all_pairs(len(lens))
    clean = _Launch(L.ALIGN_DTW, SE.EUCLID, _Side(A, "frame"), _Side(B, "frame"), pairs, back=True, path=True)
    # the records of the empty sequences point behind their buffers: nothing of them may be read
    for side in (clean.sa, clean.sb):
        side.host["base"][[0, 3]] = side.flat.numel() + 1000
        side.table.copy_(_dev(side.host.view(np.uint8).reshape(-1).copy()))
    cost, steps, bad = clean.run().results()
    want = [SE.dtw(A[a], B[b], SE.EUCLID, want_back=True) for a, b in pairs]
    assert bad == 0
    _check_against(want, cost, steps)
    for p, (a, b) in enumerate(pairs):
        if lens[a] == 0 or lens[b] == 0:
            assert np.isposinf(cost[p]) and steps[p] == 0
    # a planted NaN (A side, a row of the second strip) and a planted inf (B side)
    A2, B2 = [a.copy() for a in A], [b.copy() for b in B]
    A2[2][68, 1], B2[4][0, 3] = np.nan, np.inf
    hurt = _Launch(L.ALIGN_DTW, SE.EUCLID, _Side(A2, "frame"), _Side(B2, "frame"), pairs, back=True, path=True).run()
    c2, s2, bad2 = hurt.results()
    is_bad = [(a == 2 and lens[b] > 0) or (b == 4 and lens[a] > 0) for a, b in pairs]
    assert bad2 == sum(is_bad)
    for p in range(len(pairs)):
        if is_bad[p]:
            assert np.isnan(c2[p]) and s2[p] == 0
            if lens[pairs[p][0]] and lens[pairs[p][1]]:
                assert (hurt.path_of(p) == -1).all()
        else:
            assert c2[p:p + 1].tobytes() == cost[p:p + 1].tobytes() and s2[p] == steps[p]
            if lens[pairs[p][0]] and lens[pairs[p][1]]:
                assert hurt.path_of(p).tobytes() == clean.path_of(p).tobytes()


# ---- the split under max_back_bytes --------------------------------------------------------------------------------------
def test_a_call_split_by_max_back_bytes_gives_the_bits_of_the_unsplit_call():
    A, B = _seqs("normal", 5, LENS)
    a, b = [_dev(x) for x in A], [_dev(x) for x in B]
    pairs = [(i, (3 * i + 1) % len(LENS)) for i in range(len(LENS))] + [(10, 10), (9, 8)]
    whole = AL.dtw(a, b, pairs=pairs, return_path=True)
    split = AL.dtw(a, b, pairs=pairs, return_path=True, max_back_bytes=40000)
    plain = AL.dtw(a, b, pairs=pairs)
    assert len(whole._run.recs) == 1 and len(split._run.recs) > 3 and split._run.back.numel() < whole._run.back.numel()
    want = _want("normal", 5, LENS, "euclid")
    k = len(LENS)
    for al in (whole, split, plain):
        assert _bits(al.cost).tolist() == _bits(whole.cost).tolist() and al.steps.tolist() == whole.steps.tolist()
        assert al.cost.cpu().numpy().tobytes() == np.array([want[x * k + y][0] for x, y in pairs], F32).tobytes()
        assert torch.equal(al.mean, al.cost / al.steps) and int(al.bad[0]) == 0
    for p, (x, y) in enumerate(pairs):
        w = want[x * k + y]
        ref = SE.walk(w[2], w[1])[:w[1]]
        assert whole.path(p).cpu().numpy().tobytes() == ref.tobytes() == split.path(p).cpu().numpy().tobytes()
    with pytest.raises(L.AewError, match="return_path"):
        plain.path(0)


def test_dtw_and_edit_distance_do_not_synchronise_the_host():
    A, B = _seqs("normal", 3, SMALL)
    a, b = [_dev(x) for x in A], [_dev(x) for x in B]
    rs = np.random.RandomState(2)
    sa, sb = [_dev(rs.randint(0, 2, n).astype(np.int64)) for n in SMALL], [_dev(rs.randint(0, 2, n).astype(np.int64)) for n in SMALL]
    pairs = [(x, y) for x in range(len(SMALL)) for y in range(len(SMALL)) if x != y]       # 12 pairs, 3 of 129 A frames
    warm = AL.dtw(a, b, pairs=pairs), AL.dtw(a, b, pairs=pairs, return_path=True), AL.edit_distance(sa, sb, pairs=pairs, collapse=False)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                  # .item() / .cpu() / a blocking copy would raise
    try:
        al = AL.dtw(a, b, pairs=pairs)
        alp = AL.dtw(a, b, pairs=pairs, return_path=True)
        ed = AL.edit_distance(sa, sb, pairs=pairs, collapse=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for got, want in ((al, warm[0]), (alp, warm[1])):
        assert torch.equal(_bits(got.cost), _bits(want.cost)) and torch.equal(got.steps, want.steps)
        assert torch.equal(_bits(got.mean), _bits(want.mean)) and int(got.bad[0]) == 0
    assert torch.equal(alp._run.path, warm[1]._run.path) and int(alp.steps.min()) > 0
    assert torch.equal(ed.distance, warm[2].distance) and torch.equal(_bits(ed.rate), _bits(warm[2].rate))
    assert int(ed.distance.max()) > 0


# ---- refused records -----------------------------------------------------------------------------------------------------
def test_malformed_records_are_refused_with_nothing_launched():
    rs = np.random.RandomState(5)
    A = [rs.randn(n, 4).astype(F32) for n in (70, 3)]
    pairs = [(0, 1), (1, 0), (0, 0)]

    def fresh():
        return _Launch(L.ALIGN_DTW, SE.EUCLID, _Side(A, "frame"), _Side(A, "frame"), pairs, back=True, path=True)

    def edits():
        def seq_field(side, field, value):
            def go(x):
                getattr(x, side).host[field][0] = value
            return go
        yield L.E_ARG, seq_field("sa", "base", 10 ** 6)                             # base + extent behind the buffer
        yield L.E_ARG, seq_field("sb", "len", 80)                                   # extent behind the buffer
        yield L.E_ARG, seq_field("sa", "len", -1)
        yield L.E_ARG, seq_field("sb", "frame_stride", -4)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 0)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 257)
        yield L.E_ARG, lambda x: x.tp["a"].__setitem__(1, 2)                        # pair index out of range
        yield L.E_ARG, lambda x: x.tp["b"].__setitem__(2, -1)
        yield L.E_ARG, lambda x: x.tp["back_base"].__setitem__(2, x.n_back - 10)    # back matrix behind the buffer
        yield L.E_ARG, lambda x: x.tp["path_base"].__setitem__(0, -1)
        yield L.E_ARG, lambda x: setattr(x.rec, "ws", None)                         # 70 A frames need the boundary rows
        yield L.E_ARG, lambda x: setattr(x.rec, "ws_bytes", 8 * 3 * 70 - 8)
        yield L.E_ARG, lambda x: setattr(x.rec, "back", None)                       # a path without back-pointers
        yield L.E_ARG, lambda x: setattr(x.rec, "mode", 2)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "feat_a", x.rec.feat_a + 2)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "cost", x.rec.cost + 1)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "path", x.rec.path + 2)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "pairs", x.rec.pairs + 4)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "ws", x.rec.ws + 1)

    n = 0
    for want_rc, edit in edits():
        x = fresh()
        edit(x)
        assert x.rc() == want_rc, n
        assert x.untouched(), n
        n += 1
    assert n == 19
    good = fresh().run()
    _, steps, _ = good.results()
    assert (steps > 0).all()


# ---- the surface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vq():
    hps, m, args = _model("vqvae-ema")
    m._ensure_engine(1)
    return hps, m, args


def _model_words(m):
    words = _engine_state(m._engine)
    assert "emb" in words and "loss_buf" in words and "ema_numer" in words
    return words


def test_code_distance_equals_the_emulator_on_the_looked_up_rows(vq):
    hps, m, _ = vq
    eng, K = m._engine, hps.bn_vq_n_embed
    before = _model_words(m)
    gen = torch.Generator().manual_seed(3)
    rows = [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in (70, 1, 33, 0, 129)]
    pairs = [(0, 4), (4, 0), (1, 2), (2, 2), (3, 0), (0, 1)]
    al = m.code_distance(rows, pairs=pairs, return_path=True)
    emb = eng.emb.reshape(K, -1)
    z = [CD.lookup(emb, r).cpu().numpy() for r in rows]
    for p, (a, b) in enumerate(pairs):
        cost, steps, back = SE.dtw(z[a], z[b], SE.EUCLID, want_back=True)
        assert al.cost[p:p + 1].cpu().numpy().tobytes() == F32(cost).tobytes() and int(al.steps[p]) == steps
        if steps:
            assert al.path(p).cpu().numpy().tobytes() == SE.walk(back, steps)[:steps].tobytes()
    assert np.isposinf(float(al.cost[4])) and float(al.mean[3]) == 0.0 and int(al.steps[3]) == 33
    sq = m.code_distance(CD.UtteranceCodes(torch.cat(rows), np.cumsum([0] + [r.numel() for r in rows])), pairs=pairs,
                         metric="sqeuclid")
    assert float(sq.cost[0]) == float(SE.dtw(z[0], z[4], SE.SQEUCLID)[0])
    after = _model_words(m)
    assert before.keys() == after.keys() and all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.code_distance([torch.tensor([0, K, 1], device=DEV)])


def test_known_answers_through_code_distance_and_edit_distance(vq):
    hps, m, _ = vq
    K = hps.bn_vq_n_embed
    emb = m._engine.emb.reshape(K, -1)
    assert torch.unique(emb, dim=0).shape[0] == K                                  # (distinct codes have distinct rows)
    base = torch.randperm(K, generator=torch.Generator().manual_seed(1))[:37].to(DEV)   # neighbouring codes differ
    twice = base.repeat_interleave(2)
    al = m.code_distance([base, twice], [twice, base, base], pairs=[(0, 0), (1, 1), (0, 2)], return_path=True)
    assert al.cost.tolist() == [0.0, 0.0, 0.0] and al.steps.tolist() == [74, 74, 37]
    assert al.path(2).cpu().tolist() == [[i, i] for i in range(37)]
    ed = AL.edit_distance([base, twice], [twice, base], collapse=True)
    assert ed.distance.tolist() == [0, 0] and ed.rate.tolist() == [0.0, 0.0] and ed.len_a.tolist() == [37, 37]
    frames = AL.edit_distance(CD.UtteranceCodes(torch.cat([base, twice]), [0, 37, 111]), pairs=[(0, 1), (1, 1)])
    assert frames.distance.tolist() == [37, 0] and frames.distance.dtype == torch.int32
    assert frames.rate.tolist() == [0.5, 0.0]
    empty = AL.edit_distance([base[:0]], [base[:0]])
    assert empty.distance.tolist() == [0] and empty.rate.tolist() == [0.0]
    assert float(AL.abx(torch.tensor([1.0, 2.0, 5.0, 4.0], device=DEV), torch.tensor([2.0, 2.0, 1.0, 5.0], device=DEV))) == 0.375


def test_cepstral_distance(vq):
    hps, m, _ = vq
    before = _model_words(m)
    gen = torch.Generator().manual_seed(5)
    w = [torch.randint(0, 256, (n,), generator=gen).float().to(DEV) for n in (4000, 5203, 700)]
    mf = m._utterance_mfcc()
    same = m.cepstral_distance([w[0]], [w[0]])
    frames = mf.ragged([CD.mu_decode(w[0], 256)])[1][0]
    assert frames > 9 and float(same.mean[0]) == 0.0 and float(same.cost[0]) == 0.0 and int(same.steps[0]) == frames
    n_mfcc = hps.n_mfcc
    for expand in (True, False):
        al = m.cepstral_distance(w[:2], w[1:], expand=expand)
        feats = [CD.mu_decode(x, 256) if expand else x for x in w]
        flat, fr, bases = mf.ragged(feats)
        flat = flat.cpu().numpy()
        cep = [flat[b:b + 3 * n_mfcc * f].reshape(3 * n_mfcc, f)[1:n_mfcc].T for b, f in zip(bases, fr)]
        for p in range(2):
            cost, steps, _ = SE.dtw(cep[p], cep[p + 1], SE.EUCLID)
            assert al.cost[p:p + 1].cpu().numpy().tobytes() == F32(cost).tobytes() and int(al.steps[p]) == steps
            assert float(al.mean[p]) == float(F32(cost) / F32(steps)) and float(al.mean[p]) > 0
    short = m.cepstral_distance([w[0], w[0][:300]], [w[0][:300], w[0][:300]])
    assert short.mean.tolist() == [float("inf")] * 2 and short.steps.tolist() == [0, 0]
    after = _model_words(m)
    assert all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)


def test_mu_decode_round_trips_every_value():
    v = torch.arange(256, device=DEV)
    x = CD.mu_decode(v, 256)
    assert torch.equal(CD.mu_encode(x, 256), v) and float(x.abs().max()) == 1.0


def test_refusals_of_the_surface():
    hps, m, _ = _model("vae")
    rows = [torch.zeros(5, dtype=torch.int64, device=DEV)]
    with pytest.raises(L.AewError, match="discrete codes"):
        m.code_distance(rows)
    with pytest.raises(L.AewError, match="discrete codes"):
        m.cepstral_distance([torch.zeros(4000, device=DEV)])
    with pytest.raises(L.AewError, match="different devices"):
        AL.dtw([torch.zeros(3, 4, device=DEV)], [torch.zeros(3, 4)])
    with pytest.raises(L.AewError, match="channels"):
        AL.dtw([torch.zeros(3, 4, device=DEV)], [torch.zeros(3, 5, device=DEV)])
    with pytest.raises(L.AewError, match="pairs"):
        AL.dtw([torch.zeros(3, 4, device=DEV)], pairs=[(0, 1)])


# ---- one plan holding the op, from a captured graph ------------------------------------------------------------------------
def test_a_captured_plan_gives_the_bits_of_the_direct_run():
    A, B = _seqs("normal", 5, LENS)
    pairs = [(8, 9), (10, 3), (0, 10), (5, 5), (9, 10)]
    x = _Launch(L.ALIGN_DTW, SE.EUCLID, _Side(A, "frame"), _Side(B, "chan"), pairs, back=True, path=True).run()
    cost, steps, _ = x.results()
    direct = (cost.tobytes(), steps.tobytes(), x.back.cpu().numpy().tobytes(), x.path.cpu().numpy().tobytes())
    p = Plan("align")
    p.add(L.OP_SEQ_ALIGN, x.rec, "seq.align")
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for rep in range(3):                                                          # capture + first launch, then two replays
        x.cost_buf.fill_(-7.0); x.steps_buf.fill_(-7); x.back_buf.fill_(9); x.path_buf.fill_(-7)
        torch.cuda.synchronize()
        p.run_graph(st)                     # (a capture succeeds only if the op neither allocates nor synchronises)
        cost, steps, _ = x.results()
        assert (cost.tobytes(), steps.tobytes(), x.back_np.tobytes(), x.path_np.tobytes()) == direct
    assert p._graph is not None
    p.invalidate_graph()
