"""AEW_OP_ABX_COUNT on the device: the op alone on raw buffers, bit for bit against the label-level restatement
(tests/abx_emulator.py) with canaries around both outputs, outputs at odd element offsets and a row pitch above N - every
lane-stride edge of B and loop edge of A, more groups than waves, one huge group beside singletons, ties, NaN, inf and an
asymmetric matrix, both modes - then refused records, a captured graph, align.distance_matrix against align.dtw, and the
surface (align.abx_score / abx_task, model.abx_codes / abx_wavs).  The kernel keeps one path for every N (the whole row
in LDS), so no N is an edge of its own."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL, codes as CD
from ae_wavenet_amd.plan import Plan
from tests import abx_emulator as AE
from tests.test_abx_cpu import MODES, SIZES, case, fresh_tables, labels, matrix, record, refusals
from tests.test_codes_gpu import _bits, _model
from tests.test_seq_align_gpu import _canaried, _dev, _intact, _model_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def _bytes(a):
    return _dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())


class _Count:
    """One launch of the op on raw buffers: the matrix with its pitch, the three tables, canaried outputs."""

    def __init__(self, D, tb):
        self.tb, self.N, self.size = tb, tb.N, tb.N * tb.G
        self.D = _dev(D)
        self.tables = (_bytes(tb.perm), _bytes(tb.groups), _bytes(tb.partner))
        self.n_buf, self.n = _canaried(self.size, torch.int32, -7)
        self.w_buf, self.w = _canaried(self.size, torch.int32, -7)
        self.rec = record(tb, tb.N, D.shape[1], self.D.data_ptr(), self.n.data_ptr(), self.w.data_ptr(),
                          tuple(t.data_ptr() for t in self.tables))

    def run(self):
        CD._run(L.OP_ABX_COUNT, self.rec, "abx count", torch.device(DEV))
        return self

    def rc(self):
        op = L.Op()
        op.kind, op.u.abx = L.OP_ABX_COUNT, self.rec
        st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
        return L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(st), None)

    def refill(self):
        self.n_buf.fill_(-7)
        self.w_buf.fill_(-7)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.n_buf == -7).all()) and bool((self.w_buf == -7).all())

    def results(self):
        torch.cuda.synchronize()
        assert _intact(self.n_buf, self.size, -7) and _intact(self.w_buf, self.size, -7), "canaries"
        shape = (self.N, self.tb.G)
        return self.n.cpu().numpy().reshape(shape), self.w.cpu().numpy().reshape(shape)


# ---- the op against the emulator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,N", [("random", 1), ("random", 2), ("random", 3), ("random", 63), ("random", 64), ("random", 65),
                                    ("random", 130), ("random", 257), ("sizes", sum(SIZES) + 128), ("huge", 1000)])
def test_counts_equal_the_emulator(kind, N, mode):
    """random: 5 categories x 3 speakers, about 15 groups for 4 waves; sizes: groups of 1, 63, 64, 65 and 129 items as A
    and as B; huge: one group of 992 items and eight singletons.  Pitch N + 3, values {0..3} with NaN and both inf."""
    D, cat, spk, tb, want_n, want_w = case(kind, N, mode, 3)
    n, w = _Count(D, tb).run().results()
    assert n.dtype == np.int32 and np.array_equal(n, want_n) and np.array_equal(w, want_w)
    assert not (n == -7).any() and not (w == -7).any()                         # every word was written
    assert not w[want_n == 0].any()                                            # and an invalid cell holds two zeros
    if N >= 63:
        assert (want_n == 0).any() and (want_n > 0).any()
    if kind == "sizes" and mode != "any":                                      # ("any" merges the two speakers' groups)
        assert {1, 63, 64, 65, 129} <= set((tb.groups["hi"] - tb.groups["lo"]).tolist())
    if kind == "random" and N >= 63:
        assert tb.G > 4


def test_rows_are_x_and_columns_are_a_and_b_on_the_device():
    D, cat, spk, tb, want_n, want_w = case("random", 130, "across", 3)
    Dt = np.full_like(D, 77)
    Dt[:, :130] = D[:, :130].T
    n, w = _Count(Dt, tb).run().results()
    e_n, e_w, cats, spks = AE.counts(Dt[:, :130], cat, spk, "across")
    assert np.array_equal(n, want_n) and not np.array_equal(w, want_w) and int(w.sum()) == int(e_w.sum())


def test_refused_records_leave_the_outputs_alone():
    D = matrix(40, 5)
    count = 0

    def device_side():
        for name in ("perm", "groups", "partner"):
            yield L.E_ARG, lambda r, tb, name=name: setattr(r, name, None)
            yield L.E_ALIGN, lambda r, tb, name=name: setattr(r, name, getattr(r, name) + 2)

    for want_rc, edit in list(refusals()) + list(device_side()):
        x = _Count(D, fresh_tables())
        edit(x.rec, x.tb)
        assert x.rc() == want_rc, count
        assert x.untouched(), count
        count += 1
    assert count == 44
    n, w = _Count(D, fresh_tables()).run().results()
    assert n.any()


def test_a_captured_plan_gives_the_counts_of_the_direct_run():
    D, cat, spk, tb, want_n, want_w = case("random", 257, "across", 3)
    x = _Count(D, tb).run()
    direct = x.results()
    p = Plan("abx")
    p.add(L.OP_ABX_COUNT, x.rec, "abx.count")
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for rep in range(3):                                                        # capture + first launch, then two replays
        x.refill()
        torch.cuda.synchronize()
        p.run_graph(st)                     # (a capture succeeds only if the op neither allocates nor synchronises)
        got = x.results()
        assert np.array_equal(got[0], direct[0]) and np.array_equal(got[1], direct[1]) and np.array_equal(got[1], want_w)
    assert p._graph is not None
    p.invalidate_graph()


# ---- distance_matrix -------------------------------------------------------------------------------------------------------
LENS = (5, 70, 0, 1, 33, 66, 12)


@pytest.fixture(scope="module")
def items():
    rs = np.random.RandomState(11)
    return [_dev(rs.randn(n, 4).astype(F32)) for n in LENS]


@pytest.mark.parametrize("value", ["mean", "cost"])
def test_distance_matrix_carries_the_bits_of_dtw(items, value):
    N = len(LENS)
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    al = AL.dtw(items, pairs=pairs)
    want = al.mean if value == "mean" else al.cost
    full = AL.distance_matrix(items, value=value)
    assert full.shape == (N, N) and full.dtype == torch.float32 and full.device.type == "cuda"
    idx = torch.tensor(pairs, device=DEV)
    assert torch.equal(_bits(full[idx[:, 0], idx[:, 1]]), _bits(want))
    assert torch.equal(_bits(full), _bits(full.T.contiguous())) and not full.diagonal().any()
    off = [j for j in range(N) if j != 2]
    assert bool(torch.isposinf(full[2, off]).all()) and bool(torch.isposinf(full[off, 2]).all())   # the empty item
    assert bool(torch.isfinite(full[off][:, off]).all())
    for max_pairs in (1, 7):
        assert torch.equal(_bits(AL.distance_matrix(items, value=value, max_pairs=max_pairs)), _bits(full))
    sq = AL.distance_matrix(items[:2], metric="sqeuclid")
    assert torch.equal(_bits(sq[0, 1:]), _bits(AL.dtw(items, pairs=[(0, 1)], metric="sqeuclid").mean))
    assert AL.distance_matrix(items[:1]).tolist() == [[0.0]]
    bad = [t.clone() for t in items]
    bad[4][7, 1] = float("nan")
    hurt = AL.distance_matrix(bad)
    assert bool(torch.isnan(hurt[4, [0, 1, 3, 5, 6]]).all()) and bool(torch.isposinf(hurt[4, 2])) and float(hurt[4, 4]) == 0.0
    with pytest.raises(L.AewError, match="max_pairs"):
        AL.distance_matrix(items, max_pairs=0)
    with pytest.raises(L.AewError, match="value must be"):
        AL.distance_matrix(items, value="steps")


# ---- the surface -----------------------------------------------------------------------------------------------------------
def test_abx_score_equals_the_emulator_end_to_end():
    D, cat, spk, tb, want_n, want_w = case("random", 130, "within", 3)
    wide = _dev(D)
    res = AL.abx_score(wide[:, :130], cat, spk, "within")                      # a view with the pitch 133, read in place
    assert np.array_equal(res.n.cpu().numpy(), want_n) and np.array_equal(res.wrong2.cpu().numpy(), want_w)
    n_e, w_e, _, _ = AE.counts(D[:, :130], cat, spk, "within")
    error, pooled, by_category, n_triples = AE.aggregate(n_e, w_e, cat, spk, "within")
    bound = tb.G ** 2 * 2.0 ** -52                                             # (derived in tests/test_abx_cpu.py)
    assert abs(float(res.error) - error) <= bound and float(res.pooled) == pooled and int(res.n_triples) == n_triples
    assert res.error.device.type == "cuda" and res.by_category.shape == (5, 5) and res.categories == tb.categories
    off = ~np.eye(130, dtype=bool)
    assert int(res.n_nan) == int(np.isnan(D[:, :130])[off].sum()) > 0
    with pytest.raises(L.AewError, match="pitch"):
        AL.abx_score(wide[:, :130].T, cat, spk)
    with pytest.raises(L.AewError, match="131 labels"):
        AL.abx_score(wide[:130, :130], list(cat) + ["c0"], list(spk) + [10])
    alone = AL.abx_score(wide[:130, :130], [3] * 130, None, "any")             # a single category: no triple, no error raised
    assert np.isnan(float(alone.error)) and int(alone.n_triples) == 0


def test_abx_score_does_not_synchronise_the_host():
    D, cat, spk, tb, want_n, want_w = case("random", 130, "across", 3)
    dist = _dev(D)[:, :130]
    warm = AL.abx_score(dist, cat, spk, "across")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                    # .item() / .cpu() / a blocking copy would raise
    try:
        res = AL.abx_score(dist, cat, spk, "across")
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(res.wrong2, warm.wrong2) and torch.equal(res.n, warm.n) and np.array_equal(res.n.cpu().numpy(), want_n)
    assert torch.equal(_bits(res.error.float()), _bits(warm.error.float())) and torch.equal(res.cells[0], warm.cells[0])


def test_abx_task_is_the_score_of_the_distance_matrix(items):
    cat, spk = ["a", "b", "a", "b", "a", "b", "a"], [0, 0, 0, 1, 1, 1, 1]
    for mode in MODES:
        whole = AL.abx_task(items, cat, spk, mode=mode, max_pairs=5)
        parts = AL.abx_score(AL.distance_matrix(items), cat, spk, mode)
        assert torch.equal(whole.wrong2, parts.wrong2) and torch.equal(whole.n, parts.n) and int(whole.n_triples) > 0
        assert float(whole.error) == float(parts.error) and float(whole.pooled) == float(parts.pooled)


def test_abx_task_and_distance_matrix_do_not_synchronise_the_host(items):
    """From the features to the score, in runs of 5 pairs (five DTW launches, five mirror writes), under torch's check."""
    cat, spk = ["a", "b", "a", "b", "a", "b", "a"], [0, 0, 0, 1, 1, 1, 1]
    warm = AL.abx_task(items, cat, spk, mode="across", max_pairs=5)
    warm_dist = AL.distance_matrix(items, value="cost")
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                    # .item() / .cpu() / a blocking copy would raise
    try:
        res = AL.abx_task(items, cat, spk, mode="across", max_pairs=5)
        dist = AL.distance_matrix(items, value="cost")
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(res.wrong2, warm.wrong2) and torch.equal(res.n, warm.n) and int(res.n_triples) > 0
    assert torch.equal(_bits(dist), _bits(warm_dist))


@pytest.fixture(scope="module")
def vq():
    hps, m, args = _model("vqvae-ema")
    m._ensure_engine(1)
    return hps, m, args


def test_abx_codes_and_abx_wavs_leave_the_model_alone(vq):
    hps, m, _ = vq
    eng, K = m._engine, hps.bn_vq_n_embed
    before = _model_words(m)
    gen = torch.Generator().manual_seed(9)
    rows = [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in (20, 7, 33, 12, 70, 5, 9, 16)]
    cat, spk = [0, 1, 0, 1, 0, 1, 0, 1], ["u", "u", "u", "u", "v", "v", "v", "v"]
    emb = eng.emb.reshape(K, -1)
    z = [CD.lookup(emb, r) for r in rows]
    for mode in ("within", "across"):
        res = m.abx_codes(rows, cat, spk, mode=mode)
        want = AL.abx_score(AL.distance_matrix(z), cat, spk, mode)
        n_e, w_e, _, _ = AE.counts(AL.distance_matrix(z).cpu().numpy(), cat, spk, mode)
        assert torch.equal(res.wrong2, want.wrong2) and torch.equal(res.n, want.n) and float(res.error) == float(want.error)
        assert int(res.n_triples) == int(n_e.sum()) == (16 if mode == "within" else 32)
        assert int(res.wrong2.sum()) == int(w_e.sum())
    same = m.abx_codes(rows, cat, None, mode="any", metric="sqeuclid", value="cost", max_pairs=3)
    assert int(same.n_triples) == 8 * 3 * 4 and 0.0 <= float(same.error) <= 1.0
    wavs = [torch.randint(0, 256, (n,), generator=gen).float().to(DEV) for n in (4000, 5000, 4500, 6000)]
    for expand in (True, False):
        res = m.abx_wavs(wavs, [0, 1, 0, 1], ["u", "u", "u", "u"], expand=expand)
        assert int(res.n_triples) == 8 and int(res.n_nan) == 0 and 0.0 <= float(res.pooled) <= 1.0
    after = _model_words(m)
    assert before.keys() == after.keys() and all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.abx_codes([torch.tensor([0, K, 1], device=DEV)] * 2, [0, 1], None, mode="any")


def test_refusals_of_the_surface():
    hps, m, _ = _model("vae")
    rows = [torch.zeros(5, dtype=torch.int64, device=DEV)] * 2
    with pytest.raises(L.AewError, match="discrete codes"):
        m.abx_codes(rows, [0, 1], None, mode="any")
    with pytest.raises(L.AewError, match="discrete codes"):
        m.abx_wavs([torch.zeros(4000, device=DEV)] * 2, [0, 1], None, mode="any")
    with pytest.raises(L.AewError, match="needs speaker labels"):
        AL.abx_score(torch.zeros(2, 2, device=DEV), [0, 1])
    with pytest.raises(L.AewError, match="GPU only"):
        AL.distance_matrix([torch.zeros(3, 4)])
