"""AEW_OP_SEQ_ALIGN without a device: the numpy emulator (tests/seq_align_emulator.py) held to definitions that share no
code with it, known answers, the tables align.py builds, the ABI mirrors and the refusals that need no GPU."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL, codes as CD
from tests import seq_align_emulator as SE

F32 = np.float32


# ---- the emulator against independent definitions -----------------------------------------------------------------------
def _lev(a, b):
    @functools.lru_cache(maxsize=None)
    def rec(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(rec(i - 1, j) + 1, rec(i, j - 1) + 1, rec(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return rec(len(a), len(b))


@pytest.mark.parametrize("alphabet", [2, 5])
def test_edit_equals_the_memoised_recursion(alphabet):
    rs = np.random.RandomState(alphabet)
    for _ in range(300):
        a = tuple(rs.randint(0, alphabet, rs.randint(0, 13)).tolist())
        b = tuple(rs.randint(0, alphabet, rs.randint(0, 13)).tolist())
        assert SE.edit(a, b) == _lev(a, b), (a, b)


def _monotone_paths(n, m):
    def rec(i, j):
        if (i, j) == (n - 1, m - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < m:
                for rest in rec(i + di, j + dj):
                    yield [(i, j)] + rest
    return rec(0, 0)


@pytest.mark.parametrize("metric", [SE.EUCLID, SE.SQEUCLID])
def test_dtw_cost_is_the_minimum_over_all_monotone_paths(metric):
    rs = np.random.RandomState(7 + metric)
    for n, m in itertools.product(range(1, 7), range(1, 7)):
        # integer-valued features: with sqeuclid every sum is exact; with euclid D = 1 makes d = |difference| exact too
        D = 3 if metric == SE.SQEUCLID else 1
        a, b = rs.randint(-4, 5, (n, D)).astype(F32), rs.randint(-4, 5, (m, D)).astype(F32)
        d = SE.local_distance(a, b, metric)
        want = min(sum(float(d[i, j]) for i, j in path) for path in _monotone_paths(n, m))
        cost, steps, back = SE.dtw(a, b, metric, want_back=True)
        assert float(cost) == want, (n, m)
        path = SE.walk(back, steps)
        _check_path(path, steps, n, m, d, cost)
        c2, s2, b2 = SE.dtw_loops(a, b, metric)
        assert (F32(c2).tobytes(), s2, b2.tobytes()) == (F32(cost).tobytes(), steps, back.tobytes())


def _check_path(path, steps, n, m, d, cost):
    assert (path[steps:] == -1).all() and path.shape == (n + m - 1, 2)
    p = path[:steps]
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (n - 1, m - 1)
    moves = {tuple(x) for x in np.diff(p, axis=0).tolist()}
    assert moves <= {(1, 1), (1, 0), (0, 1)}
    acc = F32(0)
    for e, (i, j) in enumerate(p):
        acc = d[i, j] if e == 0 else F32(d[i, j] + acc)
    assert F32(acc).tobytes() == F32(cost).tobytes()


@pytest.mark.parametrize("n,m,D,metric", [(65, 129, 13, SE.EUCLID), (37, 50, 3, SE.SQEUCLID), (1, 9, 2, SE.EUCLID),
                                          (9, 1, 2, SE.EUCLID)])
def test_the_two_emulator_forms_agree_and_the_path_reproduces_the_cost(n, m, D, metric):
    rs = np.random.RandomState(n * m)
    a, b = rs.randn(n, D).astype(F32), rs.randn(m, D).astype(F32)
    if D == 3:
        a, b = rs.randint(0, 2, (n, D)).astype(F32), rs.randint(0, 2, (m, D)).astype(F32)     # ties in most cells
    cost, steps, back = SE.dtw(a, b, metric, want_back=True)
    c2, s2, b2 = SE.dtw_loops(a, b, metric)
    assert (F32(c2).tobytes(), s2, b2.tobytes()) == (F32(cost).tobytes(), steps, back.tobytes())
    _check_path(SE.walk(back, steps), steps, n, m, SE.local_distance(a, b, metric), cost)


def test_special_pairs():
    a = np.ones((4, 2), F32)
    assert SE.dtw(a[:0], a) == (F32(np.inf), 0, None) and SE.dtw(a, a[:0])[:2] == (F32(np.inf), 0)
    for v in (np.nan, np.inf):
        b = a.copy()
        b[2, 1] = v
        cost, steps, _ = SE.dtw(a, b)
        assert np.isnan(cost) and steps == 0
    assert SE.edit([], [1, 2, 3]) == 3 and SE.edit([4], []) == 1 and SE.edit([], []) == 0


# ---- known answers -----------------------------------------------------------------------------------------------------
def stretched(n, D, seed=0):
    """(a, its two-fold time stretch): neighbouring frames of a are pairwise distinct."""
    rs = np.random.RandomState(seed)
    a = rs.randn(n, D).astype(F32)
    assert all((a[i] != a[i + 1]).any() for i in range(n - 1))
    return a, np.repeat(a, 2, axis=0)


def test_a_sequence_against_its_time_stretch_costs_nothing():
    a, b = stretched(37, 13)
    for x, y in ((a, b), (b, a)):
        cost, steps, _ = SE.dtw(x, y)
        assert (float(cost), steps) == (0.0, 74)


def test_a_sequence_against_itself_takes_the_diagonal():
    a, _ = stretched(37, 13)
    cost, steps, back = SE.dtw(a, a, want_back=True)
    assert (float(cost), steps) == (0.0, 37)
    assert SE.walk(back, steps)[:37].tolist() == [[i, i] for i in range(37)]


# ---- the tables --------------------------------------------------------------------------------------------------------
def test_pair_table_prefix_sums_and_chunks():
    la, lb = [3, 0, 70, 5], [4, 2, 0, 100]
    pairs = np.array([(0, 0), (1, 1), (2, 3), (3, 2), (3, 3), (0, 1)], np.int64)
    t, chunks, n_back, n_path, wstride = AL.pair_table(la, lb, pairs, None)
    bb, pb, nb, npth = SE.pair_bases(la, lb, pairs.tolist())
    assert t["back_base"].tolist() == bb and t["path_base"].tolist() == pb and (n_back, n_path) == (nb, npth)
    assert chunks == [(0, 6)] and wstride == [100]                       # only pair (2, 3) has more than 64 A frames
    assert t["a"].tolist() == pairs[:, 0].tolist() and t["b"].tolist() == pairs[:, 1].tolist()
    # bounded memory: back_base restarts in every chunk, path_base runs on
    t2, chunks2, n_back2, n_path2, wstride2 = AL.pair_table(la, lb, pairs, 600)
    assert chunks2 == SE.chunks(la, lb, pairs.tolist(), 600) == [(0, 2), (2, 3), (3, 6)]   # 7000 cells: a run of its own
    assert t2["path_base"].tolist() == pb and n_path2 == npth
    assert t2["back_base"].tolist() == [0, 12, 0, 0, 0, 500] and n_back2 == 7000 and wstride2 == [0, 100, 0]
    for lo, hi in chunks2:
        cells = [la[a] * lb[b] for a, b in pairs[lo:hi]]
        assert sum(cells) <= 600 or hi - lo == 1 or sum(cells[:-1]) <= 600


def test_default_pairs():
    assert AL.default_pairs(3, 3, None).tolist() == [[0, 0], [1, 1], [2, 2]]
    assert AL.default_pairs(2, None, None).tolist() == [[0, 0], [1, 1]]                    # b=None: a with itself
    assert AL.default_pairs(2, None, [(0, 1), (1, 0)]).tolist() == [[0, 1], [1, 0]]
    with pytest.raises(L.AewError, match="zipped"):
        AL.default_pairs(3, 2, None)
    for bad in ([(0, 3)], [(-1, 0)], [(2, 0)], [0, 1], np.zeros((1, 2))):
        with pytest.raises(L.AewError, match="pairs"):
            AL.default_pairs(2, 3, bad)


def test_ragged_checks_its_views_and_builds_the_records():
    flat = torch.zeros(100)
    r = AL.Ragged(flat, [0, 39], [3, 20], [13, 1], [1, 20], 3)
    t = r.table()
    assert t.dtype.itemsize == C.sizeof(L.AlignSeq) == 32
    assert t["base"].tolist() == [0, 39] and t["len"].tolist() == [3, 20]
    assert t["frame_stride"].tolist() == [13, 1] and t["chan_stride"].tolist() == [1, 20]
    assert AL.Ragged(flat, [0], [0], 1, 1, 200).length == [0]              # an empty sequence reaches nowhere
    with pytest.raises(L.AewError, match="outside its buffer"):
        AL.Ragged(flat, [0, 41], [3, 20], [13, 1], [1, 20], 3)             # 41 + 19 + 2 * 20 = 100
    with pytest.raises(L.AewError, match="strides"):
        AL.Ragged(flat, [0], [3], -1, 1, 3)


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_abi_mirrors():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert lib.aew_sizeof(46) == -1 and lib.aew_sizeof(50) == -1
    assert lib.aew_sizeof(47) == C.sizeof(L.AlignSeq) == np.dtype(L.ALIGN_SEQ_DTYPE).itemsize
    assert lib.aew_sizeof(48) == C.sizeof(L.AlignPair) == np.dtype(L.ALIGN_PAIR_DTYPE).itemsize
    assert lib.aew_sizeof(49) == C.sizeof(L.SeqAlign)
    # the op record did not grow: the union's size is still that of its largest EARLIER member
    others = max(C.sizeof(t) for n, t in L._OpU._fields_ if n != "align")
    assert C.sizeof(L.SeqAlign) <= others and C.sizeof(L.Op) == lib.aew_sizeof(0) == 16 + others
    assert L.OP_SEQ_ALIGN == 46 and L.OP_FIELD[L.OP_SEQ_ALIGN] == "align" and L.OP_SCORE_REDUCE == 45


def test_the_launcher_refuses_a_malformed_record_without_a_device():
    """The checks run on the host copies before anything is launched, so a refusal needs no GPU."""
    seq = np.zeros(1, dtype=L.ALIGN_SEQ_DTYPE)
    seq["len"], seq["frame_stride"], seq["chan_stride"] = 4, 2, 1
    pair = np.zeros(1, dtype=L.ALIGN_PAIR_DTYPE)
    feat = np.zeros(8, np.float32)
    out = np.zeros(4, np.int32)

    def rec(**over):
        r = L.SeqAlign()
        r.mode, r.metric, r.D, r.n_pairs, r.n_a, r.n_b = L.ALIGN_DTW, L.ALIGN_EUCLID, 2, 1, 1, 1
        r.seq_a = r.seq_a_host = r.seq_b = r.seq_b_host = seq.ctypes.data
        r.pairs = r.pairs_host = pair.ctypes.data
        r.feat_a = r.feat_b = feat.ctypes.data
        r.n_feat_a = r.n_feat_b = 8
        r.cost, r.steps, r.bad = out.ctypes.data, out.ctypes.data + 4, out.ctypes.data + 8
        for k, v in over.items():
            setattr(r, k, v)
        return r

    def run(r):
        op = L.Op()
        op.kind, op.u.align = L.OP_SEQ_ALIGN, r
        return L.load().aew_run_plan(C.byref(op), 1, None, None)

    for over in (dict(D=0), dict(D=257), dict(mode=2), dict(metric=2), dict(n_pairs=0), dict(n_feat_a=7), dict(n_feat_b=-1),
                 dict(cost=None), dict(pairs_host=None), dict(path=out.ctypes.data), dict(mode=L.ALIGN_EDIT, D=2),
                 dict(n_a=0)):
        assert run(rec(**over)) == L.E_ARG, over
    for over in (dict(feat_a=feat.ctypes.data + 2), dict(cost=out.ctypes.data + 1), dict(seq_a=seq.ctypes.data + 4)):
        assert run(rec(**over)) == L.E_ALIGN, over
    bad_pair = pair.copy()
    bad_pair["b"] = 1
    assert run(rec(pairs_host=bad_pair.ctypes.data)) == L.E_ARG
    neg = seq.copy()
    neg["len"] = -1
    assert run(rec(seq_b_host=neg.ctypes.data)) == L.E_ARG
    assert not out.any()


# ---- refusals of the surface that need no device -----------------------------------------------------------------------
def test_align_refuses_before_any_launch():
    a = [torch.zeros(3, 4), torch.zeros(2, 4)]
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.dtw(a)
    with pytest.raises(L.AewError, match="channels"):
        AL.dtw(a, [torch.zeros(3, 5), torch.zeros(2, 5)])
    with pytest.raises(L.AewError, match="same number of channels"):
        AL.dtw([torch.zeros(3, 4), torch.zeros(2, 5)])
    with pytest.raises(L.AewError, match="float32"):
        AL.dtw([torch.zeros(3, 4, dtype=torch.float64)])
    with pytest.raises(L.AewError, match="metric"):
        AL.dtw(a, metric="cosine")
    with pytest.raises(L.AewError, match="pairs"):
        AL.dtw(a, pairs=[(0, 2)])
    with pytest.raises(L.AewError, match=r"D must lie"):
        AL.dtw([torch.zeros(3, 257)])
    with pytest.raises(L.AewError, match="int64"):
        AL.edit_distance([torch.zeros(3, dtype=torch.int32)])
    with pytest.raises(L.AewError, match="no CPU path"):
        AL.edit_distance([torch.zeros(3, dtype=torch.int64)])
    with pytest.raises(L.AewError, match="two"):
        AL.abx(torch.zeros(3), torch.zeros(4))


def test_abx_counts_ties_one_half():
    d_ax = torch.tensor([1.0, 2.0, 3.0, 4.0])
    d_bx = torch.tensor([2.0, 2.0, 1.0, 5.0])
    assert float(AL.abx(d_ax, d_bx)) == (0 + 0.5 + 1 + 0) / 4


def test_mu_decode_inverts_mu_encode_on_every_value():
    v = torch.arange(256)
    x = CD.mu_decode(v, 256)
    assert x.dtype == torch.float32 and float(x.abs().max()) <= 1.0 and float(x[0]) == -1.0 and float(x[255]) == 1.0
    assert torch.equal(CD.mu_encode(x, 256), v)
    assert bool((x[1:] > x[:-1]).all())
