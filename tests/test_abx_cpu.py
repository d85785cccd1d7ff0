"""AEW_OP_ABX_COUNT without a GPU: aew_abx_host - the launcher's checks and the kernel's own definitions of w and of cell
validity on the CPU - against the label-level restatement (tests/abx_emulator.py), known answers, the host tables of
align.abx_tables, align.abx_aggregate on CPU tensors, the ABI mirrors and every refusal.  All counts are integers and
compared exactly; the one bound, for the fp64 aggregation, is derived at its test."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL
from tests import abx_emulator as AE

F32 = np.float32
MODES = ("within", "across", "any")


# ---- data: label sets and matrices, and their emulator counts, computed once ---------------------------------------------
def matrix(N, seed, ld=None):
    """(N, ld) fp32 with the matrix in [:, :N]: values from {0..3} so that ties are the common case, about 6 % NaN, +inf
    and -inf, asymmetric; 77 in the pitch columns."""
    rs = np.random.RandomState(seed)
    D = rs.randint(0, 4, (N, N)).astype(F32)
    hit = rs.rand(N, N)
    D[hit < 0.02], D[(hit >= 0.02) & (hit < 0.04)], D[(hit >= 0.04) & (hit < 0.06)] = np.nan, np.inf, -np.inf
    full = np.full((N, ld or N), 77, F32)
    full[:, :N] = D
    return full


@functools.lru_cache(maxsize=None)
def labels(kind, N, seed=0):
    """(category, speaker) tuples.  "random": C = 5 x S = 3 (strings and integers); "sizes": the groups of one speaker
    have SIZES items and a second speaker repeats the first three, so A and B meet every lane-stride and loop edge;
    "huge": one group of N - 8 items (the first of the nine extra items joins it) and eight singletons under three
    speakers."""
    rs = np.random.RandomState(1000 + N + seed)
    if kind == "random":
        return tuple(f"c{k}" for k in rs.randint(0, 5, N)), tuple(int(k) for k in rs.randint(10, 13, N))
    if kind == "sizes":
        cat = [k for k, n in enumerate(SIZES) for _ in range(n)] + [k for k, n in enumerate(SIZES[:3]) for _ in range(n)]
        spk = [0] * sum(SIZES) + [1] * sum(SIZES[:3])
        order = rs.permutation(len(cat))
        return tuple(cat[i] for i in order), tuple(spk[i] for i in order)
    if kind == "huge":
        cat = [0] * (N - 9) + [0, 1, 2, 1, 2, 3, 0, 3, 4]
        spk = [0] * (N - 9) + [0, 0, 0, 1, 1, 1, 2, 2, 2]
        order = rs.permutation(N)
        return tuple(cat[i] for i in order), tuple(spk[i] for i in order)
    raise ValueError(kind)


SIZES = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def case(kind, N, mode, ld_extra=0, seed=0):
    """(D with pitch N + ld_extra, category, speaker, tables, expected n (N, G), expected wrong2 (N, G)): the emulator's
    counts laid out as the op lays them out - row = sorted position, column = group - by label VALUE."""
    cat, spk = labels(kind, N, seed)
    D = matrix(N, 7 * N + seed, N + ld_extra)
    tb = AL.abx_tables(cat, spk, mode)
    n_e, w_e, cats, spks = AE.counts(D[:, :N], cat, spk, mode)
    gc = [cats.index(tb.categories[c]) for c in tb.groups["cat"]]
    gs = [spks.index(tb.speakers[s]) for s in tb.groups["spk"]]
    want_n, want_w = n_e[tb.perm][:, gc, gs], w_e[tb.perm][:, gc, gs]
    assert want_n.sum() == n_e.sum() and want_w.sum() == w_e.sum()           # (nothing lies outside the groups)
    return D, cat, spk, tb, want_n, want_w


def record(tb, N, ld, dist_ptr, n_ptr, w_ptr, dev=None):
    """An aew_abx_count_t over the host tables of tb; dev = (perm, groups, partner) device pointers or None."""
    r = L.AbxCount()
    r.mode, r.N, r.G, r.C, r.S, r.ld = tb.op_mode, N, tb.G, tb.C, tb.S, ld
    r.dist, r.n, r.wrong2 = dist_ptr, n_ptr, w_ptr
    r.perm_host, r.groups_host, r.partner_host = tb.perm.ctypes.data, tb.groups.ctypes.data, tb.partner.ctypes.data
    if dev is not None:
        r.perm, r.groups, r.partner = dev
    return r


def host_counts(D, tb):
    N = tb.N
    n, w = np.full((N, tb.G), 0xDEAD, np.uint32), np.full((N, tb.G), 0xDEAD, np.uint32)
    rc = L.load().aew_abx_host(C.byref(record(tb, N, D.shape[1], D.ctypes.data, n.ctypes.data, w.ctypes.data)))
    assert rc == 0, rc
    return n, w


def score(D, cat, spk, mode):
    """aew_abx_host + abx_aggregate on CPU tensors."""
    tb = AL.abx_tables(cat, spk, mode)
    n, w = host_counts(np.ascontiguousarray(D, F32), tb)
    return AL.abx_aggregate(torch.from_numpy(w.astype(np.int64)), torch.from_numpy(n.astype(np.int64)), tb)


# ---- the counts against the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,N,ld_extra", [("random", 1, 0), ("random", 2, 0), ("random", 3, 5), ("random", 40, 0),
                                             ("random", 65, 3), ("random", 130, 0), ("sizes", sum(SIZES) + 128, 1),
                                             ("huge", 150, 0)])
def test_host_counts_equal_the_emulator(kind, N, ld_extra, mode):
    D, cat, spk, tb, want_n, want_w = case(kind, N, mode, ld_extra)
    n, w = host_counts(D, tb)
    assert np.array_equal(n, want_n) and np.array_equal(w, want_w)
    if N >= 40:
        assert want_n.any() and (want_n == 0).any()                            # valid and invalid cells both occur
        assert ((want_w > 0) & (want_w < 2 * want_n)).any()                    # and cells that are neither all right nor all wrong


def test_rows_are_x_and_columns_are_a_and_b():
    """An asymmetric matrix: the transposed one counts differently, and the op follows the emulator on both."""
    D, cat, spk, tb, want_n, want_w = case("random", 40, "across")
    Dt = np.ascontiguousarray(D.T)
    n_t, w_t = host_counts(Dt, tb)
    e_n, e_w, cats, spks = AE.counts(Dt, cat, spk, "across")
    assert np.array_equal(n_t, want_n) and not np.array_equal(w_t, want_w)
    assert int(w_t.sum()) == int(e_w.sum())


# ---- known answers ---------------------------------------------------------------------------------------------------------
def _by_category(cat, same, other):
    c = np.asarray(cat)
    return np.where(c[:, None] == c[None, :], F32(same), F32(other))


@pytest.mark.parametrize("mode", MODES)
def test_separated_constant_and_reversed(mode):
    cat, spk = labels("random", 40)
    for D, want in ((_by_category(cat, 0, 1), 0.0), (np.full((40, 40), 2.5, F32), 0.5), (_by_category(cat, 1, 0), 1.0),
                    (np.full((40, 40), np.nan, F32), 0.5)):
        res = score(D, cat, spk, mode)
        assert float(res.error) == want and float(res.pooled) == want and int(res.n_triples) > 0
        bc = res.by_category.numpy()
        assert np.isnan(np.diag(bc)).all() and (bc[~np.isnan(bc)] == want).all()


@pytest.mark.parametrize("mode", MODES)
def test_a_single_category_has_no_triples(mode):
    res = score(matrix(12, 1), [7] * 12, [k % 3 for k in range(12)], mode)
    assert np.isnan(float(res.error)) and np.isnan(float(res.pooled)) and int(res.n_triples) == 0
    assert not res.n.any() and not res.wrong2.any() and np.isnan(res.by_category.numpy()).all()


def test_a_category_with_one_item_under_a_speaker_has_no_a():
    cat, spk = ["p", "q", "q", "p", "q"], [0, 0, 0, 1, 1]                    # "p" is alone under both speakers
    tb = AL.abx_tables(cat, spk, "within")
    n, w = host_counts(matrix(5, 2), tb)
    x_of = {int(i): x for x, i in enumerate(tb.perm)}
    assert not n[x_of[0]].any() and not n[x_of[3]].any()                       # X = the lonely item: every cell invalid
    assert n[x_of[1]].sum() == 1 and n[x_of[2]].sum() == 1 and not n[x_of[4]].any()
    across = AL.abx_tables(cat, spk, "across")                                 # A comes from the other speaker: X is never in it
    n2, _ = host_counts(matrix(5, 2), across)
    x_of = {int(i): x for x, i in enumerate(across.perm)}
    assert [int(n2[x_of[i]].sum()) for i in range(5)] == [1, 1, 1, 2, 2]


def test_one_a_and_one_b_per_cell_is_align_abx_over_the_triples():
    """Four speakers, each with two items of "x" and one each of "y" and "z", within: every valid cell is one triple."""
    cat, spk = ["x", "x", "y", "z"] * 4, [s for s in range(4) for _ in range(4)]
    D = matrix(16, 3)
    D[np.isnan(D)] = 1                                                         # (align.abx leaves a NaN out of both of its terms)
    res = score(D, cat, spk, "within")
    d_ax, d_bx = [], []
    for s in range(4):
        for x, a in ((4 * s, 4 * s + 1), (4 * s + 1, 4 * s)):
            for b in (4 * s + 2, 4 * s + 3):
                d_ax.append(D[x, a])
                d_bx.append(D[x, b])
    assert int(res.n_triples) == len(d_ax) == 16 and int(res.n.max()) == 1
    assert float(res.pooled) == float(AL.abx(torch.tensor(d_ax), torch.tensor(d_bx)))


# ---- the host tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,N", [("random", 1), ("random", 130), ("sizes", sum(SIZES) + 128), ("huge", 150)])
def test_tables_are_a_stable_sort_into_tiling_groups(kind, N, mode):
    cat, spk = labels(kind, N)
    tb = AL.abx_tables(cat, spk, mode)
    perm, groups, partner, cats, spks = tb
    assert sorted(perm.tolist()) == list(range(N)) and perm.dtype == np.int32 and partner.dtype == np.int32
    assert groups.dtype == np.dtype(L.ABX_GROUP_DTYPE) and partner.shape == (len(cats), len(spks)) == (tb.C, tb.S)
    assert groups["lo"][0] == 0 and groups["hi"][-1] == N and (groups["lo"][1:] == groups["hi"][:-1]).all()
    assert (groups["hi"] > groups["lo"]).all()
    seen = set()
    for g, (lo, hi, c, s) in enumerate(groups.tolist()):
        items = perm[lo:hi].tolist()
        assert items == sorted(items)                                          # stable: the items' own order inside a group
        assert all(cat[i] == cats[c] and (mode == "any" or spk[i] == spks[s]) for i in items)
        assert partner[c, s] == g and (c, s) not in seen
        seen.add((c, s))
    assert (partner >= 0).sum() == tb.G and np.array_equal(tb.group_of, np.repeat(np.arange(tb.G), groups["hi"] - groups["lo"]))
    keys = [(int(groups["spk"][g]), int(groups["cat"][g])) for g in range(tb.G)]
    assert keys == sorted(keys)
    if mode == "any":
        assert spks == [0] and AL.abx_tables(cat, None, "any").perm.tolist() == perm.tolist()


def test_refusals_of_the_tables():
    with pytest.raises(L.AewError, match="needs speaker labels"):
        AL.abx_tables([1, 2], None, "within")
    with pytest.raises(L.AewError, match="mode must be"):
        AL.abx_tables([1, 2], [0, 0], "both")
    with pytest.raises(L.AewError, match="2 category labels and 3 speaker labels"):
        AL.abx_tables([1, 2], [0, 0, 0], "across")
    with pytest.raises(L.AewError, match="hashable"):
        AL.abx_tables([[1], [2]], [0, 0], "across")
    with pytest.raises(L.AewError, match="at least one item"):
        AL.abx_tables([], [], "across")
    with pytest.raises(L.AewError, match="runs on the GPU only"):
        AL.abx_score(torch.zeros(3, 3), [1, 2, 1], [0, 0, 0])
    with pytest.raises(L.AewError, match="float32"):
        AL.abx_score(torch.zeros(3, 4), [1, 2, 1], [0, 0, 0])


# ---- the aggregation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,N", [("random", 130), ("huge", 150), ("sizes", sum(SIZES) + 128)])
def test_aggregate_equals_the_emulators(kind, N, mode):
    """The bound.  Every cell error is one correctly rounded fp64 quotient in [0, 1] in both computations (the same
    two integers divided), so the two differ only by the order in which the means are summed.  A sum of m numbers in
    [0, 1] taken in any order carries at most (m - 1) m 2^-53 of absolute error (each of the m - 1 additions rounds a
    partial sum <= m), so its mean carries below m 2^-53, the rounding of the quotient included.  by_category[pair] is the
    mean of the m_pair cells of that pair, error the mean of the P present pairs: its error is at most that of the worst
    by_category entry plus that of its own mean, (max m_pair + P) 2^-53.  Every present pair owns at least one of the
    cells, so max m_pair + P - 1 <= the number of cells, and cells never pair a group with one of its own category, so
    there are at most G^2 - G of them: each computation lies within G^2 2^-53 of the exact value, the two within
    G^2 2^-52 of each other."""
    D, cat, spk, tb, want_n, want_w = case(kind, N, mode)
    n_e, w_e, _, _ = AE.counts(D[:, :N], cat, spk, mode)
    error, pooled, by_category, n_triples = AE.aggregate(n_e, w_e, cat, spk, mode)
    res = AL.abx_aggregate(torch.from_numpy(want_w), torch.from_numpy(want_n), tb)
    bound = tb.G ** 2 * 2.0 ** -52
    assert res.by_category.dtype == torch.float64 and res.cells[0].dtype == torch.int64
    assert int(res.n_triples) == n_triples > 0 and int(res.cells[1].sum()) == n_triples
    assert float(res.pooled) == pooled                                         # one quotient of the same two integers
    assert abs(float(res.error) - error) <= bound, (float(res.error), error)
    got = res.by_category.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(by_category))
    assert (np.abs(got - by_category)[~np.isnan(got)] <= bound).all()
    assert 0.0 < error < 1.0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_mirrors():
    lib = L.load()
    assert lib.aew_abi_version() == 28 and lib.aew_sizeof(57) == -1 and lib.aew_sizeof(60) == -1
    assert lib.aew_sizeof(58) == C.sizeof(L.AbxGroup) == np.dtype(L.ABX_GROUP_DTYPE).itemsize == 16
    assert lib.aew_sizeof(59) == C.sizeof(L.AbxCount) == 104
    assert C.sizeof(L.Op) == lib.aew_sizeof(0) == 16 + C.sizeof(L.GemmNT) == 1656     # the op record did not grow
    assert L.OP_ABX_COUNT == L.OP_SEQ_SEARCH + 1 == 50 and L.OP_FIELD[L.OP_ABX_COUNT] == "abx"
    assert (L.ABX_WITHIN, L.ABX_ACROSS, L.ABX_MAX_N) == (0, 1, 16384) and "aew_abx_host" in L.EXPORTS


def refusals():
    """(return code, edit of (record, tables)) for every refusal the header lists; shared with the GPU test."""
    def field(name, value):
        return lambda r, tb: setattr(r, name, value)

    def table(name, field_, at, value):
        def go(r, tb):
            t = getattr(tb, name)
            (t if field_ is None else t[field_]).reshape(-1)[at] = value
        return go
    yield L.E_ARG, field("mode", 2)
    yield L.E_ARG, field("mode", -1)
    yield L.E_ARG, field("N", 0)
    yield L.E_ARG, field("N", 16385)
    yield L.E_ARG, field("N", 39)                                               # perm still holds item 39: no permutation of [0, 39)
    yield L.E_ARG, one_item_fewer                                               # a permutation of [0, 39), but the groups tile [0, 40)
    yield L.E_ARG, field("G", 0)
    yield L.E_ARG, field("G", 41)
    yield L.E_ARG, field("G", 3)
    yield L.E_ARG, field("C", 0)
    yield L.E_ARG, field("S", 0)
    yield L.E_ARG, field("C", 1 << 26)                                          # C * S > N * G
    yield L.E_ARG, lambda r, tb: setattr(r, "C", 40 * tb.G // tb.S + 1)         # the least C with C * S > N * G
    yield L.E_ARG, field("ld", 39)
    for name in ("dist", "perm_host", "groups_host", "partner_host", "n", "wrong2"):
        yield L.E_ARG, field(name, None)
    yield L.E_ARG, table("perm", None, 3, 40)
    yield L.E_ARG, table("perm", None, 3, -1)
    yield L.E_ARG, lambda r, tb: tb.perm.__setitem__(3, tb.perm[4])             # no permutation: one item twice
    yield L.E_ARG, table("groups", "lo", 0, 1)
    yield L.E_ARG, lambda r, tb: tb.groups["hi"].__setitem__(2, tb.groups["hi"][2] - 1)   # a gap
    yield L.E_ARG, lambda r, tb: tb.groups["hi"].__setitem__(tb.G - 1, 41)
    yield L.E_ARG, lambda r, tb: tb.groups["hi"].__setitem__(1, tb.groups["lo"][1])       # an empty group
    yield L.E_ARG, table("groups", "cat", 1, 5)
    yield L.E_ARG, table("groups", "spk", 1, -1)
    yield L.E_ARG, lambda r, tb: tb.groups["cat"].__setitem__(1, tb.groups["cat"][0])     # the partner table names another group
    yield L.E_ARG, lambda r, tb: tb.partner.reshape(-1).__setitem__(int(np.flatnonzero(tb.partner.reshape(-1) >= 0)[0]), -1)
    yield L.E_ARG, one_more_category                                            # an entry no group owns
    for name in ("dist", "perm_host", "groups_host", "partner_host", "n", "wrong2"):
        yield L.E_ALIGN, lambda r, tb, name=name: setattr(r, name, getattr(r, name) + 2)


def one_item_fewer(r, tb):
    """N = 39 with item 39 taken out of perm: the permutation check passes, only the tiling check is left to refuse."""
    tb.perm = np.ascontiguousarray(tb.perm[tb.perm != 39])
    r.N, r.perm_host = 39, tb.perm.ctypes.data


def one_more_category(r, tb):
    """A further row of the partner table, of a category no group has, that names group 0: every group still finds itself."""
    tb.partner = np.concatenate([tb.partner.reshape(-1), np.array([0] + [-1] * (tb.S - 1), np.int32)])
    r.C, r.partner_host = r.C + 1, tb.partner.ctypes.data


def fresh_tables():
    cat, spk = labels("random", 40)
    tb = AL.abx_tables(cat, spk, "across")
    tb.partner = np.ascontiguousarray(tb.partner)
    return tb


def test_every_refusal_and_nothing_written():
    lib = L.load()
    D = matrix(40, 5)
    assert lib.aew_abx_host(None) == L.E_ARG
    count = 0
    for want_rc, edit in refusals():
        tb = fresh_tables()
        n, w = np.full((41, 41), 0xDEAD, np.uint32), np.full((41, 41), 0xDEAD, np.uint32)
        r = record(tb, 40, 40, D.ctypes.data, n.ctypes.data, w.ctypes.data)
        edit(r, tb)
        assert lib.aew_abx_host(C.byref(r)) == want_rc, count
        assert (n == 0xDEAD).all() and (w == 0xDEAD).all(), count
        count += 1
    assert count == 38
    tb = fresh_tables()                                                         # N * G > 2^27 needs real tables: 16384 singletons
    big = AL.abx_tables(list(range(16384)), [0] * 16384, "within")
    r = record(big, 16384, 16384, D.ctypes.data, D.ctypes.data, D.ctypes.data)
    assert big.G == 16384 and lib.aew_abx_host(C.byref(r)) == L.E_ARG
    n, w = host_counts(D, tb)                                                   # and the unedited record is accepted
    assert n.any()
