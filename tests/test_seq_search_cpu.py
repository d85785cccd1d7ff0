"""AEW_OP_SEQ_SEARCH without a device: the numpy emulator (tests/seq_search_emulator.py) held to a brute force over all
paths and to the closed DTW of tests/seq_align_emulator.py on document slices, the pick's properties, known answers, the
tables align.py builds, the ABI mirrors and the refusals that need no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL
from tests import seq_align_emulator as SE, seq_search_emulator as SS

F32 = np.float32


def _draw(rs, kind, n, D):
    return rs.randint(0, 2, (n, D)).astype(F32) if kind == "binary" else rs.randn(n, D).astype(F32)


# ---- the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,D,metric,kind", [(65, 129, 13, SS.EUCLID, "normal"), (37, 50, 3, SS.SQEUCLID, "binary"),
                                               (1, 9, 2, SS.EUCLID, "normal"), (9, 1, 2, SS.EUCLID, "binary"),
                                               (17, 70, 1, SS.SQEUCLID, "binary")])
def test_the_two_emulator_forms_agree(n, m, D, metric, kind):
    rs = np.random.RandomState(n * m)
    a, b = _draw(rs, kind, n, D), _draw(rs, kind, m, D)
    one, two = SS.sweep(a, b, metric), SS.sweep_loops(a, b, metric)
    for x, y in zip(one[:3], two[:3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert one[3] is False and two[3] is False


def _paths_to(i, j):
    """All monotone paths that end at (i, j) and start anywhere in row 0 (a cell of row 0 has no predecessor)."""
    if i == 0:
        yield [(0, j)]
        return
    for di, dj in ((1, 1), (1, 0), (0, 1)):
        pi, pj = i - di, j - dj
        if pj < 0:
            continue
        for head in _paths_to(pi, pj):
            yield head + [(i, j)]


@pytest.mark.parametrize("metric", [SS.EUCLID, SS.SQEUCLID])
def test_the_end_cost_is_the_minimum_over_all_monotone_paths_from_row_0(metric):
    rs = np.random.RandomState(11 + metric)
    for n, m in itertools.product(range(1, 5), range(1, 6)):
        # integer-valued features: with sqeuclid every sum is exact; with euclid D = 1 makes d = |difference| exact too
        D = 3 if metric == SS.SQEUCLID else 1
        a, b = rs.randint(-4, 5, (n, D)).astype(F32), rs.randint(-4, 5, (m, D)).astype(F32)
        d = SS.local_distance(a, b, metric)
        ec, es, eb, bad = SS.sweep(a, b, metric)
        assert not bad
        for j in range(m):
            paths = list(_paths_to(n - 1, j))
            costs = [sum(float(d[c]) for c in p) for p in paths]
            assert float(ec[j]) == min(costs), (n, m, j)
            # the (steps, start) the sweep reports belong to one of the cheapest paths
            assert (int(es[j]), int(eb[j])) in {(len(p), p[0][1]) for p, c in zip(paths, costs) if c == min(costs)}


@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_every_end_cost_is_the_closed_dtw_of_the_query_against_its_slice(kind):
    """The slice property: C(n-1, j) equals, bit for bit, AEW_OP_SEQ_ALIGN's cost of a against b[B : j + 1]; the steps
    agree wherever no tie decides the path (continuous data)."""
    rs = np.random.RandomState(5 if kind == "normal" else 6)
    ends = 0
    for D, metric, n, m in ((1, SS.EUCLID, 5, 40), (3, SS.SQEUCLID, 17, 70), (12, SS.EUCLID, 9, 33), (3, SS.EUCLID, 1, 12),
                            (1, SS.SQEUCLID, 13, 7)):
        a, b = _draw(rs, kind, n, D), _draw(rs, kind, m, D)
        ec, es, eb, _ = SS.sweep(a, b, metric)
        for j in range(m):
            s = int(eb[j])
            assert 0 <= s <= j
            cost, steps, _ = SE.dtw(a, b[s:j + 1], metric)
            assert F32(cost).tobytes() == ec[j:j + 1].tobytes(), (D, metric, j)
            if kind == "normal":
                assert steps == int(es[j])
            ends += 1
    assert ends == 162


def test_special_pairs():
    a = np.ones((4, 2), F32)
    (ec, es, eb), hits, cost, steps, count, bad = SS.search(a[:0], a, n_hits=2)
    assert np.isposinf(ec).all() and ec.size == 4 and not es.any() and (eb == -1).all() and (count, bad) == (0, False)
    assert (hits == -1).all() and np.isposinf(cost).all() and not steps.any()
    (ec, es, eb), hits, cost, steps, count, bad = SS.search(a, a[:0])
    assert ec.size == es.size == eb.size == 0 and (count, bad) == (0, False) and (hits == -1).all()
    for v in (np.nan, np.inf):
        b = a.copy()
        b[2, 1] = v
        (ec, es, eb), hits, cost, steps, count, bad = SS.search(a, b)
        assert np.isnan(ec).all() and not es.any() and (eb == -1).all() and (count, bad) == (0, True)
        assert (hits == -1).all() and np.isposinf(cost).all()


# ---- the pick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [SS.MEAN, SS.COST])
@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_pick_properties(kind, rank):
    rs = np.random.RandomState(3 + rank)
    a, b = _draw(rs, kind, 6, 2), _draw(rs, kind, 90, 2)
    ec, es, eb, _ = SS.sweep(a, b)
    key = SS.keys(ec, es, rank)
    hits, cost, steps, count = SS.pick(ec, es, eb, 32, rank)
    assert 1 < count < 32                                                     # 90 frames hold fewer than 32 disjoint matches
    assert (hits[count:] == -1).all() and np.isposinf(cost[count:]).all() and not steps[count:].any()
    got = [key[e] for _, e in hits[:count]]
    assert got == sorted(got) and got[0] == key.min() and hits[0, 1] == int(np.argmin(key))
    iv = sorted((int(s), int(e)) for s, e in hits[:count])
    assert all(s <= e for s, e in iv) and all(iv[q][1] < iv[q + 1][0] for q in range(count - 1))      # disjoint
    for r in range(count):
        s, e = hits[r]
        assert s == eb[e] and cost[r] == ec[e] and steps[r] == es[e]
    # nothing eligible was left: every end overlaps a hit
    assert all(any(eb[k] <= e and k >= s for s, e in iv) for k in range(90))
    # a shorter list is a prefix of a longer one
    h3 = SS.pick(ec, es, eb, 3, rank)
    assert h3[0].tobytes() == hits[:3].tobytes() and h3[3] == 3


def test_min_len_max_len_and_the_two_ranks():
    rs = np.random.RandomState(9)
    a, b = rs.randn(8, 3).astype(F32), rs.randn(120, 3).astype(F32)
    ec, es, eb, _ = SS.sweep(a, b)
    length = np.arange(120) - eb + 1
    assert length.min() < 4 < length.max()                                    # (the limits below cut into what exists)
    for lo, hi in ((4, 0), (1, 6), (5, 9), (200, 0)):
        hits, cost, steps, count = SS.pick(ec, es, eb, 32, SS.MEAN, lo, hi)
        ln = hits[:count, 1] - hits[:count, 0] + 1
        assert (ln >= lo).all() and (hi == 0 or (ln <= hi).all())
        ok = (length >= lo) & ((length <= hi) if hi else True)
        assert count == 0 if not ok.any() else hits[0, 1] == int(np.argmin(np.where(ok, SS.keys(ec, es), np.inf)))
    by_mean, by_cost = SS.pick(ec, es, eb, 1, SS.MEAN), SS.pick(ec, es, eb, 1, SS.COST)
    assert by_cost[0][0, 1] == int(np.argmin(ec)) and by_mean[0][0, 1] == int(np.argmin(ec / es.astype(F32)))
    # ties go to the least end: three equal keys
    tie = SS.pick(np.array([2, 1, 1, 1], F32), np.ones(4, np.int32), np.arange(4, dtype=np.int32), 4, SS.COST)
    assert tie[0][:, 1].tolist() == [1, 2, 3, 0]
    # a key that is not finite is never a hit
    inf = SS.pick(np.array([np.inf, 3], F32), np.ones(2, np.int32), np.arange(2, dtype=np.int32), 2, SS.COST)
    assert inf[3] == 1 and inf[0].tolist() == [[1, 1], [-1, -1]]


@pytest.mark.parametrize("metric", [SS.EUCLID, SS.SQEUCLID])
def test_a_query_cut_from_the_document_is_hit_0(metric):
    rs = np.random.RandomState(21)
    b = rs.randn(200, 5).astype(F32)
    for s, e in ((0, 0), (17, 30), (150, 199), (64, 128)):
        _, hits, cost, steps, count, bad = SS.search(b[s:e + 1].copy(), b, metric, n_hits=3)
        assert hits[0].tolist() == [s, e] and float(cost[0]) == 0.0 and steps[0] == e - s + 1 and count >= 1 and not bad


# ---- the tables --------------------------------------------------------------------------------------------------------
def test_search_pair_table_prefix_sums():
    lq, ld = [3, 0, 70, 65], [4, 2, 0, 100]
    pairs = np.array([(0, 0), (1, 1), (2, 3), (3, 2), (3, 1), (0, 3)], np.int64)
    t, n_prof, wstride = AL.search_pair_table(lq, ld, pairs)
    bases, total = SS.prof_bases(ld, pairs.tolist())
    assert t["prof_base"].tolist() == bases == [0, 4, 6, 106, 106, 108] and n_prof == total == 208
    assert wstride == SS.ws_stride(lq, ld, pairs.tolist()) == 100
    assert t["a"].tolist() == pairs[:, 0].tolist() and t["b"].tolist() == pairs[:, 1].tolist()
    assert AL.search_pair_table(lq, ld, pairs[:2])[2] == 0                     # no query of more than 64 frames


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_abi_mirrors():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert lib.aew_sizeof(54) == -1 and lib.aew_sizeof(57) == -1
    assert lib.aew_sizeof(55) == C.sizeof(L.SearchPair) == np.dtype(L.SEARCH_PAIR_DTYPE).itemsize == 16
    assert lib.aew_sizeof(56) == C.sizeof(L.SeqSearch)
    assert C.sizeof(L.Op) == lib.aew_sizeof(0) == 1656                         # the op record did not grow
    assert L.OP_SEQ_SEARCH == L.OP_CODE_SEGMENT + 1 == 49 and L.OP_FIELD[L.OP_SEQ_SEARCH] == "search"
    assert (L.SEARCH_MEAN, L.SEARCH_COST, L.SEARCH_MAX_HITS) == (SS.MEAN, SS.COST, SS.MAX_HITS) == (0, 1, 32)


def test_the_launcher_refuses_a_malformed_record_without_a_device():
    """The checks run on the host copies before anything is launched, so a refusal needs no GPU."""
    seq = np.zeros(2, dtype=L.ALIGN_SEQ_DTYPE)
    seq["len"], seq["frame_stride"], seq["chan_stride"] = 4, 2, 1
    long_q = seq.copy()
    long_q["len"][0], long_q["frame_stride"][0], long_q["chan_stride"][0] = 70, 0, 0   # 70 query frames that fit 8 elements
    pair = np.zeros(1, dtype=L.SEARCH_PAIR_DTYPE)
    feat = np.zeros(8, np.float32)
    out = np.zeros(64, np.int32)

    def rec(**over):
        r = L.SeqSearch()
        r.metric, r.rank, r.D, r.n_pairs, r.n_a, r.n_b = L.ALIGN_EUCLID, L.SEARCH_MEAN, 2, 1, 2, 2
        r.n_hits, r.min_len, r.max_len = 3, 1, 0
        r.seq_a = r.seq_a_host = r.seq_b = r.seq_b_host = seq.ctypes.data
        r.pairs = r.pairs_host = pair.ctypes.data
        r.feat_a = r.feat_b = feat.ctypes.data
        r.n_feat_a = r.n_feat_b = 8
        base = out.ctypes.data
        r.prof_cost, r.prof_steps, r.prof_start, r.n_prof = base, base + 16, base + 32, 4
        r.hits, r.hit_cost, r.hit_steps, r.count, r.bad = base + 48, base + 72, base + 84, base + 96, base + 100
        for k, v in over.items():
            setattr(r, k, v)
        return r

    def run(r):
        op = L.Op()
        op.kind, op.u.search = L.OP_SEQ_SEARCH, r
        return L.load().aew_run_plan(C.byref(op), 1, None, None)

    outputs = ("prof_cost", "prof_steps", "prof_start", "hits", "hit_cost", "hit_steps", "count", "bad")
    for over in [dict(n_hits=0), dict(n_hits=33), dict(rank=2), dict(rank=-1), dict(metric=2), dict(D=0), dict(D=257),
                 dict(n_pairs=0), dict(n_a=0), dict(min_len=-1), dict(max_len=-1), dict(n_feat_a=7), dict(n_feat_b=-1),
                 dict(pairs_host=None), dict(seq_b=None), dict(n_prof=3), dict(n_prof=-1)] + [{k: None} for k in outputs]:
        assert run(rec(**over)) == L.E_ARG, over
    for base in (-1, 1, 1 << 40):                                             # prof_base outside n_prof
        moved = pair.copy()
        moved["prof_base"] = base
        assert run(rec(pairs_host=moved.ctypes.data)) == L.E_ARG, base
    bad_pair = pair.copy()
    bad_pair["b"] = 2
    assert run(rec(pairs_host=bad_pair.ctypes.data)) == L.E_ARG
    neg = seq.copy()
    neg["len"][0] = -1
    assert run(rec(seq_b_host=neg.ctypes.data)) == L.E_ARG
    # a query of more than 64 frames: no workspace, then one that is 4 bytes short of 12 * pairs * m
    assert run(rec(seq_a_host=long_q.ctypes.data)) == L.E_ARG
    assert run(rec(seq_a_host=long_q.ctypes.data, ws=out.ctypes.data + 128, ws_bytes=12 * 4 - 4)) == L.E_ARG
    for over in (dict(feat_a=feat.ctypes.data + 2), dict(hit_cost=out.ctypes.data + 1), dict(seq_a=seq.ctypes.data + 4),
                 dict(prof_start=out.ctypes.data + 2), dict(count=out.ctypes.data + 3)):
        assert run(rec(**over)) == L.E_ALIGN, over
    assert not out.any()


# ---- refusals of the surface that need no device -----------------------------------------------------------------------
def test_search_refuses_before_any_launch():
    a = [torch.zeros(3, 4), torch.zeros(2, 4)]
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.search(a)
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.search(a, [torch.zeros(9, 4), torch.zeros(5, 4)], n_hits=2)
    with pytest.raises(L.AewError, match="channels"):
        AL.search(a, [torch.zeros(3, 5), torch.zeros(2, 5)])
    with pytest.raises(L.AewError, match="float32"):
        AL.search([torch.zeros(3, 4, dtype=torch.float64)])
    with pytest.raises(L.AewError, match="metric"):
        AL.search(a, metric="cosine")
    with pytest.raises(L.AewError, match="rank"):
        AL.search(a, rank="median")
    for n_hits in (0, 33):
        with pytest.raises(L.AewError, match="n_hits"):
            AL.search(a, n_hits=n_hits)
    with pytest.raises(L.AewError, match="min_len"):
        AL.search(a, min_len=-1)
    with pytest.raises(L.AewError, match="pairs"):
        AL.search(a, pairs=[(0, 2)])
    with pytest.raises(L.AewError, match=r"D must lie"):
        AL.search([torch.zeros(3, 257)])
