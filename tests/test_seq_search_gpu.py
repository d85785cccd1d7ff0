"""AEW_OP_SEQ_SEARCH on the device: the op alone, bit for bit against its numpy restatement (tests/seq_search_emulator.py)
with canaries around every output and outputs at odd element offsets - every strip and 64-column edge, every register
instantiation of D, both layouts, ties, the pick's controls, empty and non-finite pairs, refused records - then every hit
against align.dtw on the device, the surface (align.search, model.search_codes / search_wavs) and one plan replayed from
a captured graph."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL, codes as CD
from ae_wavenet_amd.plan import Plan
from tests import seq_search_emulator as SS
from tests.test_codes_gpu import _bits, _model
from tests.test_seq_align_gpu import _Side, _canaried, _dev, _intact, _model_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
QLENS = (1, 2, 63, 64, 65, 129)
DLENS = (1, 2, 63, 64, 65, 129, 257)
SMALL = (1, 63, 65, 129)
METRIC = {"euclid": SS.EUCLID, "sqeuclid": SS.SQEUCLID}


# ---- data sets and their emulator results, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seqs(kind, D, qlens, dlens):
    rs = np.random.RandomState(D * 1000 + len(qlens) + (7 if kind == "binary" else 0))
    draw = (lambda n: rs.randint(0, 2, (n, D)).astype(F32)) if kind == "binary" else (lambda n: rs.randn(n, D).astype(F32))
    return [draw(n) for n in qlens], [draw(n) for n in dlens]


def _grid(nq, nd):
    return [(a, b) for a in range(nq) for b in range(nd)]


@functools.lru_cache(maxsize=None)
def _want(kind, D, qlens, dlens, metric, n_hits=1, rank=SS.MEAN, min_len=1, max_len=0):
    A, B = _seqs(kind, D, qlens, dlens)
    return [SS.search(A[a], B[b], METRIC[metric], n_hits, rank, min_len, max_len) for a, b in _grid(len(qlens), len(dlens))]


# ---- one launch of the op on raw buffers ---------------------------------------------------------------------------------
class _Search:
    OUTS = (("prof_cost", torch.float32), ("prof_steps", torch.int32), ("prof_start", torch.int32), ("hits", torch.int32),
            ("hit_cost", torch.float32), ("hit_steps", torch.int32), ("count", torch.int32))

    def __init__(self, metric, sa, sb, pairs, n_hits=1, rank=SS.MEAN, min_len=1, max_len=0):
        self.sa, self.sb, self.pairs, self.H = sa, sb, pairs, n_hits
        tp, n_prof, wstride = AL.search_pair_table(sa.lens, sb.lens, np.asarray(pairs, np.int64))
        self.tp, self.P, self.n_prof = tp, len(pairs), n_prof
        self.d_tp = _dev(tp.view(np.uint8).reshape(-1).copy())
        P, H = self.P, n_hits
        self.size = dict(prof_cost=max(n_prof, 1), prof_steps=max(n_prof, 1), prof_start=max(n_prof, 1), hits=2 * P * H,
                         hit_cost=P * H, hit_steps=P * H, count=P)
        self.buf, self.out = {}, {}
        for name, dt in self.OUTS:
            self.buf[name], self.out[name] = _canaried(self.size[name], dt, -7)
        self.bad = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(3 * P * wstride, dtype=torch.float32, device=DEV) if wstride else None
        r = self.rec = L.SeqSearch()
        r.metric, r.rank, r.D, r.n_pairs = metric, rank, sa.D, P
        r.n_hits, r.min_len, r.max_len = n_hits, min_len, max_len
        r.seq_a, r.seq_a_host, r.n_a = sa.table.data_ptr(), sa.host.ctypes.data, len(sa.host)
        r.seq_b, r.seq_b_host, r.n_b = sb.table.data_ptr(), sb.host.ctypes.data, len(sb.host)
        r.pairs, r.pairs_host = self.d_tp.data_ptr(), tp.ctypes.data
        r.feat_a, r.n_feat_a, r.feat_b, r.n_feat_b = sa.flat.data_ptr(), sa.flat.numel(), sb.flat.data_ptr(), sb.flat.numel()
        for name, _ in self.OUTS:
            setattr(r, name, self.out[name].data_ptr())
        r.n_prof, r.bad = n_prof, self.bad.data_ptr()
        if self.ws is not None:
            r.ws, r.ws_bytes = self.ws.data_ptr(), 4 * self.ws.numel()

    def run(self):
        CD._run(L.OP_SEQ_SEARCH, self.rec, "seq search", torch.device(DEV))
        return self

    def rc(self):
        op = L.Op()
        op.kind, op.u.search = L.OP_SEQ_SEARCH, self.rec
        st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        return L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(st), None)

    def refill(self):
        for b in self.buf.values():
            b.fill_(-7)
        self.bad.zero_()

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((b == -7).all()) for b in self.buf.values()) and not bool(self.bad.any())

    def results(self):
        """{name: numpy array} after the canary checks; "bad" the count."""
        torch.cuda.synchronize()
        for name, _ in self.OUTS:
            assert _intact(self.buf[name], self.size[name], -7), f"canaries around {name}"
        assert not self.bad[1:].any()
        got = {name: self.out[name].cpu().numpy() for name, _ in self.OUTS}
        got["bad"] = int(self.bad[0].item()) & 0xFFFFFFFF
        return got

    def same_as(self, got, want):
        """Every output of every pair against the emulator's (profile, hits, cost, steps, count, bad) tuples."""
        H = self.H
        for p, ((a, b), w) in enumerate(zip(self.pairs, want)):
            lo, m = int(self.tp["prof_base"][p]), self.sb.lens[b]
            for name, ref in zip(("prof_cost", "prof_steps", "prof_start"), w[0]):
                assert got[name][lo:lo + m].tobytes() == ref.tobytes(), (name, p, (a, b))
            assert got["hits"][2 * H * p:2 * H * (p + 1)].tobytes() == w[1].tobytes(), ("hits", p, (a, b))
            assert got["hit_cost"][H * p:H * (p + 1)].tobytes() == w[2].tobytes(), ("hit_cost", p, (a, b))
            assert got["hit_steps"][H * p:H * (p + 1)].tobytes() == w[3].tobytes(), ("hit_steps", p, (a, b))
            assert got["count"][p] == w[4], ("count", p, (a, b))
        assert got["bad"] == sum(bool(w[5]) for w in want)


# ---- the op against the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_search_equals_the_emulator_on_every_strip_and_column_edge(kind, metric):
    """All 42 (query, document) pairs of QLENS x DLENS in one launch, three hits each; then the channel-major view of the
    same values and a mixed one.  The binary features put ties in most cells."""
    A, B = _seqs(kind, 3, QLENS, DLENS)
    want = _want(kind, 3, QLENS, DLENS, metric, 3)
    pairs = _grid(len(QLENS), len(DLENS))
    first = _Search(METRIC[metric], _Side(A, "frame"), _Side(B, "frame"), pairs, n_hits=3).run()
    got = first.results()
    first.same_as(got, want)
    assert got["count"].max() == 3 and got["count"].min() == 1
    for la, lb in (("chan", "chan"), ("chan", "frame")):
        other = _Search(METRIC[metric], _Side(A, la), _Side(B, lb), pairs, n_hits=3).run()
        g2 = other.results()
        assert all(g2[k].tobytes() == got[k].tobytes() for k, _ in _Search.OUTS) and g2["bad"] == 0


@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("D", [1, 4, 5, 8, 12, 13, 16, 17, 32, 33, 64, 65, 256])
def test_search_equals_the_emulator_for_every_way_D_is_held(D, metric):
    A, B = _seqs("normal", D, SMALL, SMALL)
    want = _want("normal", D, SMALL, SMALL, metric)
    pairs = _grid(len(SMALL), len(SMALL))
    outs = []
    for layout in ("frame", "chan"):
        run = _Search(METRIC[metric], _Side(A, layout), _Side(B, layout), pairs).run()
        got = run.results()
        run.same_as(got, want)
        outs.append([got[k].tobytes() for k, _ in _Search.OUTS])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("n_hits,rank,min_len,max_len", [(1, SS.MEAN, 1, 0), (3, SS.COST, 1, 0), (32, SS.MEAN, 1, 0),
                                                         (32, SS.COST, 4, 0), (3, SS.MEAN, 3, 9), (32, SS.MEAN, 1, 5),
                                                         (3, SS.COST, 300, 0)])
@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_the_pick_controls(kind, n_hits, rank, min_len, max_len):
    qlens, dlens = (5, 70), (200, 257, 3)
    A, B = _seqs(kind, 4, qlens, dlens)
    want = _want(kind, 4, qlens, dlens, "euclid", n_hits, rank, min_len, max_len)
    pairs = _grid(2, 3)
    run = _Search(SS.EUCLID, _Side(A, "frame"), _Side(B, "frame"), pairs, n_hits, rank, min_len, max_len).run()
    got = run.results()
    run.same_as(got, want)
    counts = got["count"].tolist()
    if min_len == 300:
        assert counts == [0] * 6                                              # nothing is that long: every slot is padding
    elif n_hits == 32:
        assert max(counts[2::3]) <= 3                                         # 3 document frames hold no more: padding slots
    else:
        assert max(counts) == n_hits


# ---- special pairs -------------------------------------------------------------------------------------------------------
def test_empty_and_non_finite_pairs():
    rs = np.random.RandomState(3)
    lens = (0, 5, 70, 0, 66)
    A = [rs.randn(n, 4).astype(F32) for n in lens]
    B = [rs.randn(n, 4).astype(F32) for n in lens]
    pairs = _grid(5, 5)
    clean = _Search(SS.EUCLID, _Side(A, "frame"), _Side(B, "frame"), pairs, n_hits=2)
    # the records of the empty sequences point behind their buffers: nothing of them may be read
    for side in (clean.sa, clean.sb):
        side.host["base"][[0, 3]] = side.flat.numel() + 1000
        side.table.copy_(_dev(side.host.view(np.uint8).reshape(-1).copy()))
    got = clean.run().results()
    want = [SS.search(A[a], B[b], SS.EUCLID, 2) for a, b in pairs]
    clean.same_as(got, want)
    assert got["bad"] == 0
    for p, (a, b) in enumerate(pairs):
        if lens[a] == 0 or lens[b] == 0:
            assert got["count"][p] == 0 and (got["hits"][4 * p:4 * p + 4] == -1).all()
            assert np.isposinf(got["hit_cost"][2 * p:2 * p + 2]).all() and not got["hit_steps"][2 * p:2 * p + 2].any()
    # a planted NaN (query side, a row of the second strip) and a planted inf (document side)
    A2, B2 = [a.copy() for a in A], [b.copy() for b in B]
    A2[2][68, 1], B2[4][0, 3] = np.nan, np.inf
    hurt = _Search(SS.EUCLID, _Side(A2, "frame"), _Side(B2, "frame"), pairs, n_hits=2).run()
    g2 = hurt.results()
    want2 = [SS.search(A2[a], B2[b], SS.EUCLID, 2) for a, b in pairs]
    hurt.same_as(g2, want2)
    is_bad = [(a == 2 and lens[b] > 0) or (b == 4 and lens[a] > 0) for a, b in pairs]
    assert g2["bad"] == sum(is_bad) == 5
    for p, (a, b) in enumerate(pairs):
        lo, m = int(hurt.tp["prof_base"][p]), lens[b]
        if is_bad[p]:                                                         # the sweep's entries were overwritten
            assert np.isnan(g2["prof_cost"][lo:lo + m]).all() and not g2["prof_steps"][lo:lo + m].any()
            assert (g2["prof_start"][lo:lo + m] == -1).all() and g2["count"][p] == 0
        else:
            assert g2["prof_cost"][lo:lo + m].tobytes() == got["prof_cost"][lo:lo + m].tobytes()


# ---- the hits against the closed DTW, on the device --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("normal", "euclid"), ("binary", "sqeuclid")])
def test_every_hit_costs_what_dtw_gives_for_its_slice(kind, metric):
    A, B = _seqs(kind, 3, QLENS, DLENS)
    q, d = [_dev(x) for x in A], [_dev(x) for x in B]
    pairs = _grid(len(QLENS), len(DLENS))
    mt = AL.search(q, d, pairs=pairs, metric=metric, n_hits=3)
    assert mt.start.shape == mt.end.shape == mt.cost.shape == mt.steps.shape == mt.mean.shape == (42, 3)
    count, start, end = mt.count.cpu().numpy(), mt.start.cpu().numpy(), mt.end.cpu().numpy()
    assert int(mt.bad[0]) == 0 and len(mt) == 42
    # one Ragged over the documents' buffer: a sequence per hit, the frames [start, end] of its document, read in place
    flat = torch.cat([x.reshape(-1) for x in d])
    doc_base = np.concatenate([[0], np.cumsum([3 * n for n in DLENS])])
    cut, who = [], []
    for p, (a, b) in enumerate(pairs):
        for r in range(count[p]):
            cut.append((int(doc_base[b]) + 3 * int(start[p, r]), int(end[p, r] - start[p, r] + 1)))
            who.append((p, r, a))
    assert len(cut) > 60
    slices = AL.Ragged(flat, [c[0] for c in cut], [c[1] for c in cut], 3, 1, 3)
    al = AL.dtw(q, slices, pairs=[(a, k) for k, (_, _, a) in enumerate(who)], metric=metric)
    idx = torch.tensor([(p, r) for p, r, _ in who], device=DEV)
    assert torch.equal(_bits(al.cost), _bits(mt.cost[idx[:, 0], idx[:, 1]]))
    if kind == "normal":                                                      # (no ties: the paths are the same ones)
        assert torch.equal(al.steps, mt.steps[idx[:, 0], idx[:, 1]])
    # the surface's own outputs are the emulator's, and profile() cuts the right views without waiting
    want = _want(kind, 3, QLENS, DLENS, metric, 3)
    for p in (0, 6, 20, 41):
        pc, ps, pb = mt.profile(p)
        assert pc.cpu().numpy().tobytes() == want[p][0][0].tobytes() and ps.cpu().numpy().tobytes() == want[p][0][1].tobytes()
        assert pb.cpu().numpy().tobytes() == want[p][0][2].tobytes()
        assert np.stack([start[p], end[p]], 1).astype(np.int32).tobytes() == want[p][1].tobytes()
        assert mt.cost[p].cpu().numpy().tobytes() == want[p][2].tobytes() and count[p] == want[p][4]
    assert torch.equal(_bits(mt.mean), _bits(mt.cost / mt.steps))


def test_a_query_cut_from_the_document_is_found_where_it_was_cut():
    rs = np.random.RandomState(21)
    doc = rs.randn(300, 12).astype(F32)
    cuts = [(0, 0), (17, 30), (150, 299), (64, 128), (100, 229)]
    mt = AL.search([_dev(doc[s:e + 1].copy()) for s, e in cuts], [_dev(doc)], pairs=[(k, 0) for k in range(len(cuts))])
    assert mt.start[:, 0].tolist() == [s for s, _ in cuts] and mt.end[:, 0].tolist() == [e for _, e in cuts]
    assert mt.cost[:, 0].tolist() == [0.0] * 5 and mt.steps[:, 0].tolist() == [e - s + 1 for s, e in cuts]
    assert mt.count.tolist() == [1] * 5


def test_search_and_profile_do_not_synchronise_the_host():
    A, B = _seqs("normal", 3, QLENS, DLENS)
    q, d = [_dev(x) for x in A], [_dev(x) for x in B]
    pairs = _grid(len(QLENS), len(DLENS))
    warm = AL.search(q, d, pairs=pairs, n_hits=3)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                  # .item() / .cpu() / a blocking copy would raise
    try:
        mt = AL.search(q, d, pairs=pairs, n_hits=3)
        prof = mt.profile(41)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(mt.start, warm.start) and torch.equal(mt.end, warm.end) and torch.equal(_bits(mt.cost), _bits(warm.cost))
    assert [x.numel() for x in prof] == [DLENS[-1]] * 3 and torch.equal(_bits(prof[0]), _bits(warm.profile(41)[0]))


# ---- refused records -----------------------------------------------------------------------------------------------------
def test_malformed_records_are_refused_with_nothing_written():
    rs = np.random.RandomState(5)
    A = [rs.randn(n, 4).astype(F32) for n in (70, 3)]
    pairs = [(0, 1), (1, 0), (0, 0)]

    def fresh():
        return _Search(SS.EUCLID, _Side(A, "frame"), _Side(A, "frame"), pairs, n_hits=2)

    def edits():
        def seq_field(side, field, value):
            def go(x):
                getattr(x, side).host[field][0] = value
            return go
        yield L.E_ARG, seq_field("sa", "base", 10 ** 6)                             # base + extent behind the buffer
        yield L.E_ARG, seq_field("sb", "len", 80)
        yield L.E_ARG, seq_field("sa", "len", -1)
        yield L.E_ARG, seq_field("sb", "frame_stride", -4)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 0)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 257)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_hits", 0)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_hits", 33)
        yield L.E_ARG, lambda x: setattr(x.rec, "rank", 2)
        yield L.E_ARG, lambda x: setattr(x.rec, "metric", 2)
        yield L.E_ARG, lambda x: setattr(x.rec, "max_len", -1)
        yield L.E_ARG, lambda x: x.tp["a"].__setitem__(1, 2)                        # pair index out of range
        yield L.E_ARG, lambda x: x.tp["b"].__setitem__(2, -1)
        yield L.E_ARG, lambda x: x.tp["prof_base"].__setitem__(2, x.n_prof - 69)    # the profile behind the buffer
        yield L.E_ARG, lambda x: x.tp["prof_base"].__setitem__(0, -1)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_prof", x.n_prof - 1)
        yield L.E_ARG, lambda x: setattr(x.rec, "ws", None)                         # 70 query frames need the boundary rows
        yield L.E_ARG, lambda x: setattr(x.rec, "ws_bytes", 12 * 3 * 70 - 12)
        yield L.E_ARG, lambda x: setattr(x.rec, "hits", None)
        yield L.E_ARG, lambda x: setattr(x.rec, "prof_start", None)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "feat_a", x.rec.feat_a + 2)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "prof_cost", x.rec.prof_cost + 1)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "pairs", x.rec.pairs + 4)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "ws", x.rec.ws + 1)

    n = 0
    for want_rc, edit in edits():
        x = fresh()
        edit(x)
        assert x.rc() == want_rc, n
        assert x.untouched(), n
        n += 1
    assert n == 24
    good = fresh().run().results()
    assert (good["count"] > 0).all()


# ---- the surface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vq():
    hps, m, args = _model("vqvae-ema")
    m._ensure_engine(1)
    return hps, m, args


def test_search_codes_equals_the_emulator_on_the_looked_up_rows(vq):
    hps, m, _ = vq
    eng, K = m._engine, hps.bn_vq_n_embed
    before = _model_words(m)
    gen = torch.Generator().manual_seed(3)
    docs = [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in (300, 129, 0, 40)]
    queries = [docs[0][100:170].clone(), docs[1][5:9].clone(), torch.randint(0, K, (7,), generator=gen).to(DEV), docs[3][:0]]
    pairs = [(0, 0), (1, 1), (2, 0), (2, 2), (3, 3), (1, 0), (0, 1)]
    mt = m.search_codes(queries, docs, pairs=pairs, n_hits=3)
    emb = eng.emb.reshape(K, -1)
    zq, zd = [CD.lookup(emb, r).cpu().numpy() for r in queries], [CD.lookup(emb, r).cpu().numpy() for r in docs]
    for p, (a, b) in enumerate(pairs):
        prof, hits, cost, steps, count, bad = SS.search(zq[a], zd[b], SS.EUCLID, 3)
        assert np.stack([mt.start[p].cpu().numpy(), mt.end[p].cpu().numpy()], 1).tobytes() == hits.tobytes(), p
        assert mt.cost[p].cpu().numpy().tobytes() == cost.tobytes() and mt.steps[p].cpu().numpy().tobytes() == steps.tobytes()
        assert int(mt.count[p]) == count and not bad
        assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(mt.profile(p), prof))
    assert (int(mt.start[0, 0]), int(mt.end[0, 0]), float(mt.cost[0, 0])) == (100, 169, 0.0)      # the planted ones
    assert (int(mt.start[1, 0]), int(mt.end[1, 0]), float(mt.cost[1, 0])) == (5, 8, 0.0)
    assert mt.count[3:5].tolist() == [0, 0] and int(mt.bad[0]) == 0
    by_cost = m.search_codes(queries[:2], CD.UtteranceCodes(torch.cat(docs[:2]), [0, 300, 429]), metric="sqeuclid", rank="cost",
                             min_len=2, max_len=100)
    assert by_cost.start[:, 0].tolist() == [100, 5] and by_cost.end[:, 0].tolist() == [169, 8]
    after = _model_words(m)
    assert before.keys() == after.keys() and all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.search_codes([torch.tensor([0, K, 1], device=DEV)], docs[:1])


def test_search_wavs_finds_a_planted_slice(vq):
    hps, m, _ = vq
    before = _model_words(m)
    gen = torch.Generator().manual_seed(5)
    doc = torch.randint(0, 256, (16000,), generator=gen).float().to(DEV)
    mf = m._utterance_mfcc()
    lo, n = 40 * mf.hop, 20 * mf.hop                                         # cut on a frame boundary: the slice's frame g
    last = 40 + mf.n_frames(n) - 1                                           # looks at the samples of the document's 40 + g
    other = torch.randint(0, 256, (n,), generator=gen).float().to(DEV)
    for expand in (True, False):
        mt = m.search_wavs([doc[lo:lo + n].clone(), other, doc[:300]], [doc], pairs=[(0, 0), (1, 0), (2, 0)], expand=expand,
                           min_len=10, max_len=40)
        # (every utterance has its own dB floor, and warping may trade a frame at an edge: 2 frames' slack)
        assert abs(int(mt.start[0, 0]) - 40) <= 2 and abs(int(mt.end[0, 0]) - last) <= 2, (mt.start[0], mt.end[0])
        assert mt.count.tolist() == [1, 1, 0] and int(mt.bad[0]) == 0         # (300 samples yield no frames)
        assert float(mt.mean[0, 0]) < 0.5 * float(mt.mean[1, 0])              # unrelated noise matches nowhere as well
    after = _model_words(m)
    assert all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)


def test_refusals_of_the_surface():
    hps, m, _ = _model("vae")
    rows = [torch.zeros(5, dtype=torch.int64, device=DEV)]
    with pytest.raises(L.AewError, match="discrete codes"):
        m.search_codes(rows, rows)
    with pytest.raises(L.AewError, match="discrete codes"):
        m.search_wavs([torch.zeros(4000, device=DEV)], [torch.zeros(4000, device=DEV)])
    with pytest.raises(L.AewError, match="different devices"):
        AL.search([torch.zeros(3, 4, device=DEV)], [torch.zeros(3, 4)])
    with pytest.raises(L.AewError, match="n_hits"):
        AL.search([torch.zeros(3, 4, device=DEV)], n_hits=33)


# ---- one plan holding the op, from a captured graph ------------------------------------------------------------------------
def test_a_captured_plan_gives_the_bits_of_the_direct_run():
    A, B = _seqs("normal", 3, QLENS, DLENS)
    pairs = [(5, 6), (4, 3), (0, 6), (3, 3), (5, 5)]
    x = _Search(SS.EUCLID, _Side(A, "frame"), _Side(B, "chan"), pairs, n_hits=3).run()
    direct = x.results()
    p = Plan("search")
    p.add(L.OP_SEQ_SEARCH, x.rec, "seq.search")
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for rep in range(3):                                                          # capture + first launch, then two replays
        x.refill()
        torch.cuda.synchronize()
        p.run_graph(st)                     # (a capture succeeds only if the op neither allocates nor synchronises)
        got = x.results()
        assert all(got[k].tobytes() == direct[k].tobytes() for k, _ in _Search.OUTS) and got["bad"] == 0
    assert p._graph is not None
    p.invalidate_graph()
