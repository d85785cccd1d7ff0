"""AEW_OP_SEQ_DISCOVER without a device: the numpy emulator (tests/seq_discover_emulator.py) in its two forms, held to a
brute force over all paths, known answers (a planted repeat, a repeat inside one utterance under a band), the pick's
properties, the tables align.py builds, the ABI mirrors and the refusals that need no GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL
from tests import seq_discover_emulator as SD

F32 = np.float32


def _draw(rs, kind, n, D):
    return rs.randint(0, 2, (n, D)).astype(F32) if kind == "binary" else rs.randn(n, D).astype(F32)


def _same(one, two):
    for x, y in zip(one, two):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,D,metric,kind,theta", [(65, 129, 13, SD.EUCLID, "normal", 4.5), (37, 50, 3, SD.SQEUCLID, "binary", 0.5),
                                                     (1, 9, 2, SD.EUCLID, "normal", 1.0), (9, 1, 2, SD.EUCLID, "binary", 0.75),
                                                     (17, 70, 1, SD.SQEUCLID, "binary", 0.5)])
def test_the_two_emulator_forms_agree(n, m, D, metric, kind, theta):
    rs = np.random.RandomState(n * m)
    a, b = _draw(rs, kind, n, D), _draw(rs, kind, m, D)
    one, two = SD.sweep(a, b, theta, metric), SD.sweep_loops(a, b, theta, metric)
    _same(one[:5], two[:5])
    assert one[5] is False and two[5] is False
    assert (one[0] > 0).any()                                                 # (the threshold lets something live)
    _same(SD.sweep(a, b, theta, metric, full=True)[:4], SD.sweep_loops(a, b, theta, metric, full=True)[:4])


@pytest.mark.parametrize("band", [1, 5])
@pytest.mark.parametrize("kind,theta", [("normal", 1.5), ("binary", 0.5)])
def test_the_two_emulator_forms_agree_on_a_self_pair_with_a_band(band, kind, theta):
    rs = np.random.RandomState(40 + band)
    a = _draw(rs, kind, 70, 3)
    one, two = SD.sweep(a, a, theta, SD.EUCLID, band), SD.sweep_loops(a, a, theta, SD.EUCLID, band)
    _same(one[:5], two[:5])
    H = SD.sweep(a, a, theta, SD.EUCLID, band, full=True)[0]
    assert not H[~SD.inside(70, 70, band)].any() and (H > 0).any()            # dead outside the band, alive somewhere inside
    # without a band the trivial diagonal (d = 0, every cell gains the whole threshold) swamps every row
    free = SD.sweep(a, a, theta, SD.EUCLID, 0)
    assert (free[0] >= (np.arange(70) + 1) * F32(theta)).all() and (free[0] >= one[0]).all()


def _paths_to(i, j, ok):
    """All monotone paths that end at (i, j), start anywhere and stay on cells with ok[i, j]."""
    if not ok[i, j]:
        return
    yield [(i, j)]
    for di, dj in ((1, 1), (1, 0), (0, 1)):
        pi, pj = i - di, j - dj
        if pi < 0 or pj < 0:
            continue
        for head in _paths_to(pi, pj, ok):
            yield head + [(i, j)]


@pytest.mark.parametrize("metric,band", [(SD.EUCLID, 0), (SD.SQEUCLID, 0), (SD.SQEUCLID, 1), (SD.EUCLID, 2)])
def test_the_score_is_the_maximum_over_all_monotone_paths(metric, band):
    """A definition that shares no code with the emulator: H(i, j) = max(0, max over all monotone paths that end at (i, j)
    of the gains summed in path order in fp32).  Integer-valued features and a threshold with one binary digit make every
    sum exact, so the maximum over paths and the dynamic programme agree to the bit."""
    rs = np.random.RandomState(17 + metric + band)
    cells = 0
    for n, m in itertools.product(range(1, 6), range(1, 6)):
        # with sqeuclid every distance is an integer; with euclid D = 1 makes d = |difference| an integer too
        D = 2 if metric == SD.SQEUCLID else 1
        a, b = rs.randint(-2, 3, (n, D)).astype(F32), rs.randint(-2, 3, (m, D)).astype(F32)
        theta = F32(1.5)
        g = (theta - SD.local_distance(a, b, metric)).astype(F32)
        ok = SD.inside(n, m, band)
        H, S, R, O, bad = SD.sweep(a, b, theta, metric, band, full=True)
        assert not bad
        for i, j in itertools.product(range(n), range(m)):
            best, who = F32(0), set()
            for p in _paths_to(i, j, ok):
                acc = F32(0)
                for c in p:
                    acc = F32(acc + g[c])
                if acc > best:
                    best, who = acc, set()
                if acc == best and acc > 0:
                    who.add((len(p), p[0]))
            assert H[i, j] == best, (n, m, i, j)
            if best > 0:                                                      # steps and origin belong to one of the best paths
                assert (int(S[i, j]), (int(R[i, j]), int(O[i, j]))) in who
            else:
                assert S[i, j] == 0
            cells += 1
    assert cells == 225


def test_special_pairs():
    a = np.ones((4, 2), F32)
    prof, hits, hs, hst, count, bad = SD.discover(a[:0], a, 1.0)
    assert all(x.size == 0 for x in prof) and (count, bad) == (0, False) and (hits == -1).all() and np.isnan(hs).all()
    prof, hits, hs, hst, count, bad = SD.discover(a, a[:0], 1.0, n_hits=2)
    assert prof[0].tolist() == [0] * 4 and all((x == -1).all() for x in prof[1:4]) and not prof[4].any()
    assert (count, bad) == (0, False) and (hits == -1).all() and not hst.any()
    for v in (np.nan, np.inf):
        b = a.copy()
        b[2, 1] = v
        prof, hits, hs, hst, count, bad = SD.discover(a, b, 1.0)
        assert np.isnan(prof[0]).all() and all((x == -1).all() for x in prof[1:4]) and not prof[4].any()
        assert (count, bad) == (0, True) and (hits == -1).all() and np.isnan(hs).all()
        # with band = 3 only cell (0, 3) is inside and column 2, the one that is not finite, is not looked at
        assert SD.discover(a, b, 1.0, band=3)[5] is False


# ---- known answers -----------------------------------------------------------------------------------------------------
def test_a_planted_repeat_is_hit_0():
    """Two random binary sequences (D = 8, sqeuclid) that share one planted stretch.  Frames that differ are at least 1
    apart, so with 0 < threshold < 1 only identical frames gain: hit 0 is the planted ranges, score L * threshold,
    steps L.  The seed is one for which the emulator says so - that is asserted here, it is not assumed."""
    rs = np.random.RandomState(3)
    L_, theta = 12, F32(0.5)
    a, b = _draw(rs, "binary", 60, 8), _draw(rs, "binary", 75, 8)
    b[40:40 + L_] = a[21:21 + L_]
    d = SD.local_distance(a, b, SD.SQEUCLID)
    assert theta > 0 and theta < d[d > 0].min()
    prof, hits, hs, hst, count, bad = SD.discover(a, b, theta, SD.SQEUCLID, n_hits=3)
    assert not bad and count >= 1
    assert hits[0].tolist() == [21, 21 + L_ - 1, 40, 40 + L_ - 1]
    assert hs[0] == F32(L_ * theta) and hst[0] == L_


def test_a_band_keeps_a_self_pair_off_its_diagonal_and_finds_an_internal_repeat_once():
    rs = np.random.RandomState(8)
    x = _draw(rs, "binary", 80, 8)
    x[50:60] = x[10:20]
    theta = F32(0.5)
    for band in (1, 3, 25):
        H, S, R, O, _ = SD.sweep(x, x, theta, SD.SQEUCLID, band, full=True)
        assert ((O - R)[H > 0] >= band).all()                                 # every alignment starts inside the band
        prof, hits, hs, hst, count, bad = SD.discover(x, x, theta, SD.SQEUCLID, band, n_hits=4)
        assert count >= 1 and ((hits[:count, 2] - hits[:count, 0]) >= band).all()
        assert hits[0].tolist() == [10, 19, 50, 59] and hs[0] == F32(5.0) and hst[0] == 10
        # once: no other hit touches the planted rows or is its mirror image (the lower triangle is dead)
        assert all(h[1] < 10 or h[0] > 19 for h in hits[1:count].tolist())
    # band 45 cuts the repeat (j - i = 40) away
    assert SD.discover(x, x, theta, SD.SQEUCLID, 45)[1][0].tolist() != [10, 19, 50, 59]


# ---- the pick ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,theta", [("normal", 0.9), ("binary", 0.25)])
def test_pick_properties(kind, theta):
    rs = np.random.RandomState(5)
    a, b = _draw(rs, kind, 90, 2), _draw(rs, kind, 70, 2)
    *prof, bad = SD.sweep(a, b, theta)
    score, end, row, col, steps = prof
    hits, hs, hst, count = SD.pick(*prof, n_hits=32)
    assert 1 < count < 32                                                     # n_hits larger than what exists
    assert (hits[count:] == -1).all() and np.isnan(hs[count:]).all() and not hst[count:].any()
    got = hs[:count].tolist()
    assert got == sorted(got, reverse=True) and got[0] == score.max() and hits[0, 1] == int(np.argmax(score))
    iv = sorted((int(h[0]), int(h[1])) for h in hits[:count])
    assert all(s <= e for s, e in iv) and all(iv[q][1] < iv[q + 1][0] for q in range(count - 1))      # disjoint A ranges
    for r in range(count):
        s, e, bs, be = hits[r]
        assert (s, bs, be) == (row[e], col[e], end[e]) and hs[r] == score[e] and hst[r] == steps[e]
    # nothing eligible was left: every row with a score overlaps a hit
    assert all(any(row[k] <= e and k >= s for s, e in iv) for k in range(90) if score[k] > 0)
    # a shorter list is a prefix of a longer one
    h3 = SD.pick(*prof, n_hits=3)
    assert count >= 3 and h3[0].tobytes() == hits[:3].tobytes() and h3[3] == 3


def test_min_len_max_len_and_ties():
    rs = np.random.RandomState(9)
    a, b = rs.randn(100, 3).astype(F32), rs.randn(120, 3).astype(F32)
    *prof, bad = SD.sweep(a, b, 2.0)
    score, end, row, col, steps = prof
    la, lb = np.arange(100) - row + 1, end - col + 1
    short = np.minimum(la, lb)[score > 0]
    assert short.min() < 3 < short.max()                                      # (the limits below cut into what exists)
    for lo, hi in ((3, 0), (1, 2), (2, 4), (500, 0)):
        hits, hs, hst, count = SD.pick(*prof, n_hits=32, min_len=lo, max_len=hi)
        sa, sb = hits[:count, 1] - hits[:count, 0] + 1, hits[:count, 3] - hits[:count, 2] + 1
        assert (sa >= lo).all() and (sb >= lo).all() and (hi == 0 or ((sa <= hi).all() and (sb <= hi).all()))
        ok = (score > 0) & (la >= lo) & (lb >= lo) & (((la <= hi) & (lb <= hi)) if hi else True)
        assert count == 0 if not ok.any() else hits[0, 1] == int(np.argmax(np.where(ok, score, -np.inf)))
    # ties go to the least row: three equal scores, disjoint one-row ranges
    i4 = np.arange(4, dtype=np.int32)
    tie = SD.pick(np.array([1, 2, 2, 2], F32), i4, i4, i4, np.ones(4, np.int32), n_hits=4)
    assert tie[0][:, 1].tolist() == [1, 2, 3, 0] and tie[3] == 4
    # a row where nothing ends (score 0, entries -1) is never a hit; neither is a NaN
    none = SD.pick(np.array([0, 3, np.nan], F32), np.array([-1, 1, -1], np.int32), np.array([-1, 1, -1], np.int32),
                   np.array([-1, 1, -1], np.int32), np.array([0, 1, 0], np.int32), n_hits=2)
    assert none[3] == 1 and none[0].tolist() == [[1, 1, 1, 1], [-1, -1, -1, -1]]
    # suppression is by A range: row 2's alignment starts in row 0 and so meets the hit [0, 1]
    sup = SD.pick(np.array([1, 5, 4, 3], F32), i4, np.array([0, 0, 0, 3], np.int32), i4, np.ones(4, np.int32), n_hits=4)
    assert sup[0][:sup[3], 1].tolist() == [1, 3]


# ---- the tables --------------------------------------------------------------------------------------------------------
def test_discover_pairs_and_pair_table():
    assert AL.discover_pairs(3, None, None).tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    assert AL.discover_pairs(2, 2, None).tolist() == [[0, 0], [1, 1]]
    assert AL.discover_pairs(3, None, [(2, 0)]).tolist() == [[2, 0]]
    la, lb = [3, 0, 70, 65], [4, 2, 0, 100]
    pairs = np.array([(0, 0), (1, 1), (2, 3), (3, 2), (3, 1), (0, 3)], np.int64)
    t, n_prof, wstride = AL.discover_pair_table(la, lb, pairs, np.array([0, 1, 2, 0, 0, 7]))
    bases, total = SD.prof_bases(la, pairs.tolist())
    assert t["prof_base"].tolist() == bases == [0, 3, 3, 73, 138, 203] and n_prof == total == 206
    assert wstride == SD.ws_stride(la, lb, pairs.tolist()) == 100
    assert t["a"].tolist() == pairs[:, 0].tolist() and t["b"].tolist() == pairs[:, 1].tolist()
    assert t["band"].tolist() == [0, 1, 2, 0, 0, 7]
    assert AL.discover_pair_table(la, lb, pairs[:2], np.zeros(2))[2] == 0      # no A side of more than 64 frames


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_abi_mirrors():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert lib.aew_sizeof(60) == -1 and lib.aew_sizeof(63) == -1
    assert lib.aew_sizeof(61) == C.sizeof(L.DiscoverPair) == np.dtype(L.DISCOVER_PAIR_DTYPE).itemsize == 24
    assert lib.aew_sizeof(62) == C.sizeof(L.SeqDiscover) == 224
    assert C.sizeof(L.Op) == lib.aew_sizeof(0) == 1656                         # the op record did not grow
    assert L.OP_SEQ_DISCOVER == L.OP_ABX_COUNT + 1 == 51 and L.OP_FIELD[L.OP_SEQ_DISCOVER] == "discover"
    assert SD.MAX_HITS == L.SEARCH_MAX_HITS == 32


def test_the_launcher_refuses_a_malformed_record_without_a_device():
    """The checks run on the host copies before anything is launched, so a refusal needs no GPU."""
    seq = np.zeros(2, dtype=L.ALIGN_SEQ_DTYPE)
    seq["len"], seq["frame_stride"], seq["chan_stride"] = 4, 2, 1
    long_a = seq.copy()
    long_a["len"][0], long_a["frame_stride"][0], long_a["chan_stride"][0] = 70, 0, 0   # 70 A frames that fit 8 elements
    pair = np.zeros(1, dtype=L.DISCOVER_PAIR_DTYPE)
    feat = np.zeros(8, np.float32)
    out = np.zeros(64, np.int32)

    def rec(**over):
        r = L.SeqDiscover()
        r.metric, r.n_hits, r.D, r.n_pairs, r.n_a, r.n_b = L.ALIGN_EUCLID, 3, 2, 1, 2, 2
        r.min_len, r.max_len, r.threshold = 1, 0, 1.0
        r.seq_a = r.seq_a_host = r.seq_b = r.seq_b_host = seq.ctypes.data
        r.pairs = r.pairs_host = pair.ctypes.data
        r.feat_a = r.feat_b = feat.ctypes.data
        r.n_feat_a = r.n_feat_b = 8
        base = out.ctypes.data
        r.prof_score, r.prof_end, r.prof_row, r.prof_col, r.prof_steps, r.n_prof = base, base + 16, base + 32, base + 48, base + 64, 4
        r.hits, r.hit_score, r.hit_steps, r.count, r.bad = base + 80, base + 128, base + 140, base + 152, base + 156
        for k, v in over.items():
            setattr(r, k, v)
        return r

    def run(r):
        op = L.Op()
        op.kind, op.u.discover = L.OP_SEQ_DISCOVER, r
        return L.load().aew_run_plan(C.byref(op), 1, None, None)

    outputs = ("prof_score", "prof_end", "prof_row", "prof_col", "prof_steps", "hits", "hit_score", "hit_steps", "count", "bad")
    for over in [dict(n_hits=0), dict(n_hits=33), dict(metric=2), dict(metric=-1), dict(D=0), dict(D=257), dict(n_pairs=0),
                 dict(n_pairs=(1 << 24) + 1), dict(n_a=0), dict(n_b=0), dict(min_len=-1), dict(max_len=-1),
                 dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=float("-inf")),
                 dict(n_feat_a=7), dict(n_feat_b=-1), dict(pairs_host=None), dict(seq_b=None), dict(n_prof=3),
                 dict(n_prof=-1)] + [{k: None} for k in outputs]:
        assert run(rec(**over)) == L.E_ARG, over
    for base in (-1, 1, 1 << 40):                                             # prof_base outside n_prof
        moved = pair.copy()
        moved["prof_base"] = base
        assert run(rec(pairs_host=moved.ctypes.data)) == L.E_ARG, base
    for band in (-1, -(1 << 31)):
        banded = pair.copy()
        banded["band"] = band
        assert run(rec(pairs_host=banded.ctypes.data)) == L.E_ARG, band
    bad_pair = pair.copy()
    bad_pair["b"] = 2
    assert run(rec(pairs_host=bad_pair.ctypes.data)) == L.E_ARG
    neg = seq.copy()
    neg["len"][0] = -1
    assert run(rec(seq_b_host=neg.ctypes.data)) == L.E_ARG
    far = seq.copy()
    far["base"][1] = 1                                                        # the sequence leaves its feature array
    far_pair = pair.copy()
    far_pair["a"] = 1
    assert run(rec(seq_a_host=far.ctypes.data, pairs_host=far_pair.ctypes.data)) == L.E_ARG
    # an A side of more than 64 frames: no workspace, then one that is 4 bytes short of 16 * pairs * m; its profile
    # would also need 70 entries
    assert run(rec(seq_a_host=long_a.ctypes.data, n_prof=70)) == L.E_ARG
    assert run(rec(seq_a_host=long_a.ctypes.data, n_prof=70, ws=out.ctypes.data + 160, ws_bytes=16 * 4 - 4)) == L.E_ARG
    assert run(rec(seq_a_host=long_a.ctypes.data, n_prof=69, ws=out.ctypes.data + 160, ws_bytes=16 * 4)) == L.E_ARG
    for over in (dict(feat_a=feat.ctypes.data + 2), dict(hit_score=out.ctypes.data + 1), dict(seq_a=seq.ctypes.data + 4),
                 dict(prof_col=out.ctypes.data + 2), dict(count=out.ctypes.data + 3)):
        assert run(rec(**over)) == L.E_ALIGN, over
    assert not out.any()


# ---- refusals of the surface that need no device -----------------------------------------------------------------------
def test_discover_refuses_before_any_launch():
    a = [torch.zeros(3, 4), torch.zeros(2, 4)]
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.discover(a, threshold=1.0)
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.discover(a, [torch.zeros(9, 4), torch.zeros(5, 4)], threshold=1.0, n_hits=2)
    with pytest.raises(L.AewError, match="channels"):
        AL.discover(a, [torch.zeros(3, 5), torch.zeros(2, 5)], threshold=1.0)
    with pytest.raises(L.AewError, match="float32"):
        AL.discover([torch.zeros(3, 4, dtype=torch.float64)], threshold=1.0)
    with pytest.raises(L.AewError, match="metric"):
        AL.discover(a, threshold=1.0, metric="cosine")
    for n_hits in (0, 33):
        with pytest.raises(L.AewError, match="n_hits"):
            AL.discover(a, threshold=1.0, n_hits=n_hits)
    for th in (None, float("nan"), float("inf"), 1e39):
        with pytest.raises(L.AewError, match="threshold"):
            AL.discover(a, threshold=th)
    with pytest.raises(L.AewError, match="min_len"):
        AL.discover(a, threshold=1.0, min_len=-1)
    with pytest.raises(L.AewError, match="band"):
        AL.discover(a, threshold=1.0, band=-1)
    with pytest.raises(L.AewError, match="pairs"):
        AL.discover(a, threshold=1.0, pairs=[(0, 2)])
    with pytest.raises(L.AewError, match=r"D must lie"):
        AL.discover([torch.zeros(3, 257)], threshold=1.0)
