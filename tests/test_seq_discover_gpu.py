"""AEW_OP_SEQ_DISCOVER on the device: the op alone, bit for bit against its numpy restatement
(tests/seq_discover_emulator.py) with canaries around every output - every strip and 64-column edge, every register
instantiation of D, both layouts, ties, bands that cross a strip, empty and non-finite pairs, records that do not fit -
then every hit against align.dtw on the device, the surface (align.discover, model.discover_codes / discover_wavs) and
one plan replayed from a captured graph."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, align as AL, codes as CD
from ae_wavenet_amd.plan import Plan
from tests import seq_discover_emulator as SD
from tests.test_codes_gpu import _bits, _model
from tests.test_seq_align_gpu import _Side, _canaried, _dev, _intact, _model_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
LENS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
METRIC = {"euclid": SD.EUCLID, "sqeuclid": SD.SQEUCLID}
# thresholds that let a part of the cells gain: about half the typical distance of normal frames, under the least
# distance (1) of binary frames that differ
THETA = {("normal", "euclid"): 1.2, ("normal", "sqeuclid"): 2.5, ("binary", "euclid"): 0.75, ("binary", "sqeuclid"): 0.75}


# ---- data sets and their emulator results, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seqs(kind, D, alens, blens):
    rs = np.random.RandomState(D * 1000 + len(alens) + (7 if kind == "binary" else 0))
    draw = (lambda n: rs.randint(0, 2, (n, D)).astype(F32)) if kind == "binary" else (lambda n: rs.randn(n, D).astype(F32))
    return [draw(n) for n in alens], [draw(n) for n in blens]


def _grid(na, nb):
    return [(a, b) for a in range(na) for b in range(nb)]


@functools.lru_cache(maxsize=None)
def _want(kind, D, alens, blens, metric, theta, n_hits=3, min_len=1, max_len=0):
    A, B = _seqs(kind, D, alens, blens)
    return [SD.discover(A[a], B[b], theta, METRIC[metric], 0, n_hits, min_len, max_len) for a, b in _grid(len(alens), len(blens))]


# ---- one launch of the op on raw buffers ---------------------------------------------------------------------------------
class _Discover:
    PROF = ("prof_score", "prof_end", "prof_row", "prof_col", "prof_steps")
    OUTS = (("prof_score", torch.float32), ("prof_end", torch.int32), ("prof_row", torch.int32), ("prof_col", torch.int32),
            ("prof_steps", torch.int32), ("hits", torch.int32), ("hit_score", torch.float32), ("hit_steps", torch.int32),
            ("count", torch.int32))

    def __init__(self, metric, theta, sa, sb, pairs, bands=None, n_hits=3, min_len=1, max_len=0):
        self.sa, self.sb, self.pairs, self.H = sa, sb, pairs, n_hits
        bands = np.zeros(len(pairs), np.int64) if bands is None else np.asarray(bands, np.int64)
        tp, n_prof, wstride = AL.discover_pair_table(sa.lens, sb.lens, np.asarray(pairs, np.int64), bands)
        self.tp, self.P, self.n_prof, self.wstride = tp, len(pairs), n_prof, wstride
        self.d_tp = _dev(tp.view(np.uint8).reshape(-1).copy())
        P, H = self.P, n_hits
        self.size = dict(prof_score=max(n_prof, 1), prof_end=max(n_prof, 1), prof_row=max(n_prof, 1), prof_col=max(n_prof, 1),
                         prof_steps=max(n_prof, 1), hits=4 * P * H, hit_score=P * H, hit_steps=P * H, count=P)
        self.buf, self.out = {}, {}
        for name, dt in self.OUTS:
            self.buf[name], self.out[name] = _canaried(self.size[name], dt, -7)
        self.bad = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(4 * P * wstride, dtype=torch.float32, device=DEV) if wstride else None
        r = self.rec = L.SeqDiscover()
        r.metric, r.n_hits, r.D, r.n_pairs = metric, n_hits, sa.D, P
        r.min_len, r.max_len, r.threshold = min_len, max_len, theta
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
        CD._run(L.OP_SEQ_DISCOVER, self.rec, "seq discover", torch.device(DEV))
        return self

    def rc(self):
        op = L.Op()
        op.kind, op.u.discover = L.OP_SEQ_DISCOVER, self.rec
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

    def same_as(self, got, want, skip=()):
        """Every output of every pair against the emulator's (profile, hits, score, steps, count, bad) tuples."""
        H = self.H
        for p, ((a, b), w) in enumerate(zip(self.pairs, want)):
            if p in skip:
                continue
            lo, n = int(self.tp["prof_base"][p]), self.sa.lens[a]
            for name, ref in zip(self.PROF, w[0]):
                assert got[name][lo:lo + n].tobytes() == ref.tobytes(), (name, p, (a, b))
            assert got["hits"][4 * H * p:4 * H * (p + 1)].tobytes() == w[1].tobytes(), ("hits", p, (a, b))
            assert got["hit_score"][H * p:H * (p + 1)].tobytes() == w[2].tobytes(), ("hit_score", p, (a, b))
            assert got["hit_steps"][H * p:H * (p + 1)].tobytes() == w[3].tobytes(), ("hit_steps", p, (a, b))
            assert got["count"][p] == w[4], ("count", p, (a, b))
        assert got["bad"] == sum(bool(w[5]) for p, w in enumerate(want) if p not in skip)

    def left_alone(self, got, p):
        """Nothing of pair p was written: its profile range, hits and count still hold the canary."""
        lo, n = int(self.tp["prof_base"][p]), self.sa.lens[self.pairs[p][0]]
        H = self.H
        return (all((got[name][lo:lo + n] == -7).all() for name in self.PROF) and (got["hits"][4 * H * p:4 * H * (p + 1)] == -7).all()
                and (got["hit_score"][H * p:H * (p + 1)] == -7).all() and (got["hit_steps"][H * p:H * (p + 1)] == -7).all()
                and got["count"][p] == -7)


# ---- the op against the emulator ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_discover_equals_the_emulator_on_every_strip_and_column_edge(kind, metric):
    """All 81 pairs of LENS x LENS in one launch, three hits each; then the channel-major view of the same values and a
    mixed one.  The binary features put ties in most cells."""
    theta = THETA[kind, metric]
    A, B = _seqs(kind, 3, LENS, LENS)
    want = _want(kind, 3, LENS, LENS, metric, theta)
    pairs = _grid(len(LENS), len(LENS))
    first = _Discover(METRIC[metric], theta, _Side(A, "frame"), _Side(B, "frame"), pairs).run()
    got = first.results()
    first.same_as(got, want)
    assert got["count"].max() == 3 and got["bad"] == 0
    for la, lb in (("chan", "chan"), ("chan", "frame")):
        other = _Discover(METRIC[metric], theta, _Side(A, la), _Side(B, lb), pairs).run()
        g2 = other.results()
        assert all(g2[k].tobytes() == got[k].tobytes() for k, _ in _Discover.OUTS) and g2["bad"] == 0


@pytest.mark.parametrize("metric", ["euclid", "sqeuclid"])
@pytest.mark.parametrize("D", [1, 12, 64, 65, 256])
def test_discover_equals_the_emulator_for_every_way_D_is_held(D, metric):
    """D = 1 and 12 sit on two rungs of the ladder, 64 on its last, 65 and 256 take the path that holds no row in
    registers.  The threshold sits a tenth under the typical distance of D normal channels, sqrt(2 D) or 2 D."""
    lens = (5, 64, 70)
    theta = float(F32(0.9 * np.sqrt(2.0 * D) if metric == "euclid" else 1.8 * D))
    A, B = _seqs("normal", D, lens, lens)
    want = _want("normal", D, lens, lens, metric, theta)
    pairs = _grid(3, 3)
    outs = []
    for layout in ("frame", "chan"):
        run = _Discover(METRIC[metric], theta, _Side(A, layout), _Side(B, layout), pairs).run()
        got = run.results()
        run.same_as(got, want)
        assert got["count"].max() >= 1
        outs.append([got[k].tobytes() for k, _ in _Discover.OUTS])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_a_band_on_self_pairs_that_crosses_a_strip(kind):
    """Self pairs of 64, 65 and 130 frames under the bands 1, 7, 64 and 65, the longest with a planted internal repeat 65
    frames on; beside them the same sequences against each other without a band."""
    lens, bands = (64, 65, 130), (1, 7, 64, 65)
    theta = THETA[kind, "euclid"]
    A, _ = _seqs(kind, 3, lens, lens)
    A = [x.copy() for x in A]
    A[2][70:90] = A[2][5:25]
    pairs = [(u, u) for u in range(3) for _ in bands] + [(0, 2), (2, 1)]
    bd = [b for _ in range(3) for b in bands] + [0, 0]
    want = [SD.discover(A[a], A[b], theta, SD.EUCLID, band, 3, 2, 0) for (a, b), band in zip(pairs, bd)]
    side = _Side(A, "frame")
    run = _Discover(SD.EUCLID, theta, side, side, pairs, bd, 3, 2, 0).run()
    got = run.results()
    run.same_as(got, want)
    for p, ((a, b), band) in enumerate(zip(pairs, bd)):
        k = got["count"][p]
        h = got["hits"][12 * p:12 * p + 4 * k].reshape(k, 4)
        assert band == 0 or ((h[:, 2] - h[:, 0]) >= band).all()               # b_start - a_start: never under the band
    # the planted repeat lies 65 frames on, inside every one of the bands: with continuous features hit 0 starts with it
    if kind == "normal":
        for p in range(8, 12):
            assert got["hits"][12 * p:12 * p + 4][[0, 2]].tolist() == [5, 70] and got["hits"][12 * p + 1] >= 24
    # 64 frames under the bands 64 and 65, 65 frames under 65: no cell is inside; 65 frames under 64: the one cell (0, 64)
    assert got["count"][[2, 3, 7]].tolist() == [0, 0, 0]
    lo = int(run.tp["prof_base"][3])
    assert (got["prof_score"][lo:lo + 64] == 0).all() and (got["prof_end"][lo:lo + 64] == -1).all()


@pytest.mark.parametrize("n_hits,min_len,max_len", [(1, 1, 0), (3, 1, 0), (32, 1, 0), (32, 2, 0), (3, 2, 6), (32, 1, 3), (3, 300, 0)])
@pytest.mark.parametrize("kind", ["normal", "binary"])
def test_the_pick_controls(kind, n_hits, min_len, max_len):
    """The pick under every one of its controls, 9 pairs in one launch: one hit, the default three, all 32 slots (hits
    held in the registers of lanes up to 31, and padding behind the hits of the pairs that have fewer), both length
    bounds, and a min_len nothing reaches."""
    alens, blens = (5, 70, 200), (200, 129, 3)
    theta = THETA[kind, "euclid"]
    A, B = _seqs(kind, 3, alens, blens)
    want = _want(kind, 3, alens, blens, "euclid", theta, n_hits, min_len, max_len)
    run = _Discover(SD.EUCLID, theta, _Side(A, "frame"), _Side(B, "frame"), _grid(3, 3), None, n_hits, min_len, max_len).run()
    got = run.results()
    run.same_as(got, want)
    counts = got["count"].tolist()
    if min_len == 300:
        assert counts == [0] * 9                                              # nothing is that long: every slot is padding
    elif (n_hits, min_len, max_len) == (32, 1, 0):
        assert max(counts) == 32 and min(counts) < 32                         # full pairs and padded ones in one launch


# ---- special pairs -------------------------------------------------------------------------------------------------------
def test_a_bad_pair_and_empty_pairs_beside_ordinary_ones():
    rs = np.random.RandomState(3)
    lens = (0, 5, 70, 0, 66)
    A = [rs.randn(n, 4).astype(F32) for n in lens]
    B = [rs.randn(n, 4).astype(F32) for n in lens]
    pairs = _grid(5, 5)
    clean = _Discover(SD.EUCLID, 1.5, _Side(A, "frame"), _Side(B, "frame"), pairs, n_hits=2)
    # the records of the empty sequences point behind their buffers: nothing of them may be read
    for side in (clean.sa, clean.sb):
        side.host["base"][[0, 3]] = side.flat.numel() + 1000
        side.table.copy_(_dev(side.host.view(np.uint8).reshape(-1).copy()))
    got = clean.run().results()
    want = [SD.discover(A[a], B[b], 1.5, SD.EUCLID, 0, 2) for a, b in pairs]
    clean.same_as(got, want)
    assert got["bad"] == 0
    for p, (a, b) in enumerate(pairs):
        if lens[a] == 0 or lens[b] == 0:
            assert got["count"][p] == 0 and (got["hits"][8 * p:8 * p + 8] == -1).all()
            assert np.isnan(got["hit_score"][2 * p:2 * p + 2]).all() and not got["hit_steps"][2 * p:2 * p + 2].any()
    # ONE bad pair: a NaN frame in a row of the second strip of A[2], reached through one pair only
    A2 = [a.copy() for a in A]
    A2.append(A[2].copy())
    A2[5][68, 1] = np.nan
    pairs2 = pairs + [(5, 4)]
    hurt = _Discover(SD.EUCLID, 1.5, _Side(A2, "frame"), _Side(B, "frame"), pairs2, n_hits=2).run()
    g2 = hurt.results()
    want2 = want + [SD.discover(A2[5], B[4], 1.5, SD.EUCLID, 0, 2)]
    hurt.same_as(g2, want2)
    assert g2["bad"] == 1 and want2[-1][5] is True
    lo = int(hurt.tp["prof_base"][25])
    assert np.isnan(g2["prof_score"][lo:lo + 70]).all() and (g2["prof_end"][lo:lo + 70] == -1).all()
    assert g2["count"][25] == 0 and (g2["hits"][200:208] == -1).all() and np.isnan(g2["hit_score"][50:52]).all()
    assert not g2["hit_steps"][50:52].any()
    # its neighbours in the launch are untouched: every other pair has the bits of the clean launch
    n_clean = clean.n_prof
    for name, _ in _Discover.OUTS:
        k = dict(hits=200, hit_score=50, hit_steps=50, count=25).get(name, n_clean)
        assert g2[name][:k].tobytes() == got[name][:k].tobytes(), name


# ---- records that do not fit ---------------------------------------------------------------------------------------------
def test_malformed_records_are_refused_with_nothing_written():
    rs = np.random.RandomState(5)
    A = [rs.randn(n, 4).astype(F32) for n in (70, 3)]
    pairs = [(0, 1), (1, 0), (0, 0)]

    def fresh():
        return _Discover(SD.EUCLID, 1.5, _Side(A, "frame"), _Side(A, "frame"), pairs, n_hits=2)

    def edits():
        def seq_field(side, field, value):
            def go(x):
                getattr(x, side).host[field][0] = value
            return go
        yield L.E_ARG, seq_field("sa", "base", 10 ** 6)                             # the sequence leaves its feature array
        yield L.E_ARG, seq_field("sb", "len", 80)
        yield L.E_ARG, seq_field("sa", "len", -1)
        yield L.E_ARG, seq_field("sb", "frame_stride", -4)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 0)
        yield L.E_ARG, lambda x: setattr(x.rec, "D", 257)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_hits", 0)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_hits", 33)
        yield L.E_ARG, lambda x: setattr(x.rec, "metric", 2)
        yield L.E_ARG, lambda x: setattr(x.rec, "max_len", -1)
        yield L.E_ARG, lambda x: setattr(x.rec, "threshold", float("nan"))
        yield L.E_ARG, lambda x: setattr(x.rec, "threshold", float("inf"))
        yield L.E_ARG, lambda x: x.tp["band"].__setitem__(1, -1)
        yield L.E_ARG, lambda x: x.tp["a"].__setitem__(1, 2)                        # pair index out of range
        yield L.E_ARG, lambda x: x.tp["b"].__setitem__(2, -1)
        yield L.E_ARG, lambda x: x.tp["prof_base"].__setitem__(2, x.n_prof - 69)    # the profile one short for this pair
        yield L.E_ARG, lambda x: x.tp["prof_base"].__setitem__(0, -1)
        yield L.E_ARG, lambda x: setattr(x.rec, "n_prof", x.n_prof - 1)             # the profile one short
        yield L.E_ARG, lambda x: setattr(x.rec, "ws", None)                         # 70 A frames need the boundary rows
        yield L.E_ARG, lambda x: setattr(x.rec, "ws_bytes", 16 * 3 * 70 - 4)        # the workspace one element short
        yield L.E_ARG, lambda x: setattr(x.rec, "hits", None)
        yield L.E_ARG, lambda x: setattr(x.rec, "prof_col", None)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "feat_a", x.rec.feat_a + 2)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "prof_score", x.rec.prof_score + 1)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "pairs", x.rec.pairs + 4)
        yield L.E_ALIGN, lambda x: setattr(x.rec, "ws", x.rec.ws + 1)

    n = 0
    for want_rc, edit in edits():
        x = fresh()
        assert x.wstride == 70 and x.rec.ws_bytes == 16 * 3 * 70
        edit(x)
        assert x.rc() == want_rc, n
        assert x.untouched(), n
        n += 1
    assert n == 26
    good = fresh().run().results()
    assert (good["count"] > 0).all()


def test_device_records_that_fail_the_checks_leave_their_pair_alone():
    """The header's second line of defence: the kernels repeat the checks on the DEVICE copies of the tables and leave a
    failing pair alone.  The host copies here are sound (the launcher accepts the record); each device copy has one record
    spoiled - a pair index out of range, a profile range one entry behind the buffer, a negative band, a B side one frame
    longer than the workspace was sized for.  The spoiled pair keeps its canaries, its neighbours get the emulator's
    bits, and no address is formed from the spoiled record (the canaries around every buffer hold)."""
    rs = np.random.RandomState(6)
    A = [rs.randn(n, 4).astype(F32) for n in (70, 3, 66)]
    B = [rs.randn(n, 4).astype(F32) for n in (10, 40)]
    pairs = [(0, 0), (1, 1), (2, 0)]
    want = [SD.discover(A[a], B[b], 1.5, SD.EUCLID, 0, 2) for a, b in pairs]

    def spoil_pairs(field, p, value):
        def go(x):
            t = x.tp.copy()
            t[field][p] = value
            x.d_tp.copy_(_dev(t.view(np.uint8).reshape(-1).copy()))
        return go

    def longer_b(x):                                                          # 11 frames, still inside the feature array
        t = x.sb.host.copy()
        t["len"][0] = 11
        x.sb.table.copy_(_dev(t.view(np.uint8).reshape(-1).copy()))

    cases = [(spoil_pairs("a", 1, 3), (1,)), (spoil_pairs("b", 2, -1), (2,)), (spoil_pairs("band", 0, -1), (0,)),
             (lambda x: spoil_pairs("prof_base", 2, x.n_prof - 65)(x), (2,)), (longer_b, (0, 2))]
    for spoil, alone in cases:
        x = _Discover(SD.EUCLID, 1.5, _Side(A, "frame"), _Side(B, "frame"), pairs, n_hits=2)
        assert x.wstride == 10
        spoil(x)
        got = x.run().results()
        x.same_as(got, want, skip=alone)
        assert all(x.left_alone(got, p) for p in alone), alone


# ---- the hits against the closed DTW, on the device --------------------------------------------------------------------------
@pytest.mark.parametrize("metric,D", [("sqeuclid", 3), ("euclid", 1)])
def test_closed_dtw_of_a_hit_costs_no_more_than_the_hit(metric, D):
    """For every emitted hit, align.dtw(a[a_start : a_end + 1], b[b_start : b_end + 1]).cost <= steps * threshold - score:
    the right side is the summed local distance along the hit's own path, which is one of the paths closed DTW minimises
    over on that rectangle, so DTW can only be cheaper or equal.  Binary features (sqeuclid, or euclid with D = 1) and a
    threshold of 0.75 make every sum on both sides exact, so the inequality is held without a tolerance."""
    theta = 0.75
    A, B = _seqs("binary", D, LENS, LENS)
    a, b = [_dev(x) for x in A], [_dev(x) for x in B]
    pairs = _grid(len(LENS), len(LENS))
    rp = AL.discover(a, b, pairs=pairs, threshold=theta, metric=metric, n_hits=3)
    assert rp.a_start.shape == rp.b_end.shape == rp.score.shape == rp.steps.shape == rp.mean.shape == (81, 3)
    assert int(rp.bad[0]) == 0 and len(rp) == 81
    count = rp.count.cpu().numpy()
    h = [x.cpu().numpy() for x in (rp.a_start, rp.a_end, rp.b_start, rp.b_end)]
    fa, fb = torch.cat([x.reshape(-1) for x in a]), torch.cat([x.reshape(-1) for x in b])
    base = np.concatenate([[0], np.cumsum([D * n for n in LENS])])
    cut_a, cut_b, who = [], [], []
    for p, (u, v) in enumerate(pairs):
        for r in range(count[p]):
            cut_a.append((int(base[u]) + D * int(h[0][p, r]), int(h[1][p, r] - h[0][p, r] + 1)))
            cut_b.append((int(base[v]) + D * int(h[2][p, r]), int(h[3][p, r] - h[2][p, r] + 1)))
            who.append((p, r))
    assert len(who) > 100
    ra = AL.Ragged(fa, [c[0] for c in cut_a], [c[1] for c in cut_a], D, 1, D)
    rb = AL.Ragged(fb, [c[0] for c in cut_b], [c[1] for c in cut_b], D, 1, D)
    al = AL.dtw(ra, rb, metric=metric)
    idx = torch.tensor(who, device=DEV)
    score, steps = rp.score[idx[:, 0], idx[:, 1]].double(), rp.steps[idx[:, 0], idx[:, 1]].double()
    along = steps * theta - score                                             # exact in fp64: multiples of 0.25
    assert bool((al.cost.double() <= along).all())
    assert bool((al.cost.double() == along).any())                            # (and not vacuously: most hits ARE the best path)
    # the surface's own outputs are the emulator's, and profile() cuts the right views without waiting
    want = _want("binary", D, LENS, LENS, metric, theta)
    for p in (0, 8, 40, 80):
        assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(rp.profile(p), want[p][0]))
        assert np.stack([x[p] for x in h], 1).astype(np.int32).tobytes() == want[p][1].tobytes()
        assert rp.score[p].cpu().numpy().tobytes() == want[p][2].tobytes() and count[p] == want[p][4]
    assert torch.equal(_bits(rp.mean), _bits(theta - rp.score / rp.steps))


def test_default_pairs_and_bands_of_one_list_and_no_host_synchronisation():
    """b=None: every unordered pair including (u, u); the self pairs get the band max(min_len, 1), or band=, the others
    none.  The second call runs with the host forbidden to wait."""
    rs = np.random.RandomState(12)
    X = [rs.randint(0, 2, (n, 8)).astype(F32) for n in (80, 70)]
    X[0][50:60] = X[0][10:20]
    X[1][30:45] = X[0][60:75]
    x = [_dev(v) for v in X]
    warm = AL.discover(x, threshold=0.5, metric="sqeuclid", n_hits=2, min_len=3)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                  # .item() / .cpu() / a blocking copy would raise
    try:
        rp = AL.discover(x, threshold=0.5, metric="sqeuclid", n_hits=2, min_len=3)
        prof = rp.profile(0)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert [v.numel() for v in prof] == [80] * 5 and len(rp) == 3
    for p, ((u, v), band) in enumerate((((0, 0), 3), ((0, 1), 0), ((1, 1), 3))):
        w = SD.discover(X[u], X[v], 0.5, SD.SQEUCLID, band, 2, 3, 0)
        got = torch.stack([rp.a_start[p], rp.a_end[p], rp.b_start[p], rp.b_end[p]], 1).cpu().numpy()
        assert got.astype(np.int32).tobytes() == w[1].tobytes() and rp.score[p].cpu().numpy().tobytes() == w[2].tobytes()
        assert torch.equal(rp.a_start[p], warm.a_start[p]) and torch.equal(_bits(rp.score[p]), _bits(warm.score[p]))
    assert (rp.a_start[0, 0].item(), rp.a_end[0, 0].item(), rp.b_start[0, 0].item(), rp.b_end[0, 0].item()) == (10, 19, 50, 59)
    assert (rp.a_start[1, 0].item(), rp.a_end[1, 0].item(), rp.b_start[1, 0].item(), rp.b_end[1, 0].item()) == (60, 74, 30, 44)
    wide = AL.discover(x, threshold=0.5, metric="sqeuclid", n_hits=2, min_len=3, band=45)    # cuts the repeat 40 frames on
    assert wide.count.tolist() == [0, 1, 0] and torch.equal(wide.a_start[1], rp.a_start[1])


# ---- the surface -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vq():
    hps, m, args = _model("vqvae-ema")
    m._ensure_engine(1)
    return hps, m, args


def test_discover_codes_returns_a_planted_run(vq):
    hps, m, _ = vq
    eng, K = m._engine, hps.bn_vq_n_embed
    before = _model_words(m)
    emb = eng.emb.reshape(K, -1)
    dist = torch.cdist(emb.double(), emb.double())
    apart = float(dist[dist > 0].min())
    assert apart > 0
    theta = 0.5 * apart                                                       # only identical codes gain
    gen = torch.Generator().manual_seed(3)
    rows = [torch.randint(0, K, (n,), generator=gen) for n in (120, 100, 0)]
    rows[1][60:90] = rows[0][20:50]
    rows = [r.to(DEV) for r in rows]
    rp = m.discover_codes(rows, threshold=theta, n_hits=2, min_len=4)
    assert len(rp) == 6                                                       # (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    z = [CD.lookup(emb, r).cpu().numpy() if r.numel() else np.zeros((0, emb.shape[1]), F32) for r in rows]
    for p, (u, v) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        w = SD.discover(z[u], z[v], theta, SD.EUCLID, 4 if u == v else 0, 2, 4, 0)
        got = torch.stack([rp.a_start[p], rp.a_end[p], rp.b_start[p], rp.b_end[p]], 1).cpu().numpy()
        assert got.astype(np.int32).tobytes() == w[1].tobytes(), p
        assert rp.score[p].cpu().numpy().tobytes() == w[2].tobytes() and int(rp.count[p]) == w[4] and not w[5]
    a0, a1, b0, b1 = (int(x[1, 0]) for x in (rp.a_start, rp.a_end, rp.b_start, rp.b_end))
    assert a0 <= 20 and a1 >= 49 and b0 <= 60 and b1 >= 89 and a1 - a0 < 40      # the planted run (a chance frame more at most)
    assert int(rp.steps[1, 0]) >= 30 and float(rp.mean[1, 0]) < theta
    assert rp.count[[2, 4, 5]].tolist() == [0, 0, 0] and int(rp.bad[0]) == 0
    two = m.discover_codes(rows[:1], rows[1:2], threshold=theta, n_hits=2, min_len=4)
    assert torch.equal(two.a_start[0], rp.a_start[1]) and torch.equal(_bits(two.score[0]), _bits(rp.score[1]))
    after = _model_words(m)
    assert before.keys() == after.keys() and all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.discover_codes([torch.tensor([0, K, 1], device=DEV)], threshold=theta)


def test_discover_wavs_finds_a_planted_stretch(vq):
    hps, m, _ = vq
    before = _model_words(m)
    gen = torch.Generator().manual_seed(5)
    mf = m._utterance_mfcc()
    one = torch.randint(0, 256, (16000,), generator=gen).float().to(DEV)
    two = torch.randint(0, 256, (12000,), generator=gen).float().to(DEV)
    n = 20 * mf.hop
    two[25 * mf.hop:25 * mf.hop + n] = one[40 * mf.hop:40 * mf.hop + n]      # frames 40 .. of `one` are frames 25 .. of `two`
    last = mf.n_frames(n) - 1
    # the scale is the front-end's: half the mean aligned distance of the two waveforms, mostly unrelated noise
    theta = 0.5 * float(m.cepstral_distance([one], [two]).mean[0])
    rp = m.discover_wavs([one], [two], threshold=theta, n_hits=2, min_len=5)
    assert int(rp.count[0]) >= 1 and int(rp.bad[0]) == 0
    a0, a1, b0, b1 = (int(x[0, 0]) for x in (rp.a_start, rp.a_end, rp.b_start, rp.b_end))
    assert a0 <= 40 + last and a1 >= 40 and b0 <= 25 + last and b1 >= 25, (a0, a1, b0, b1)      # overlaps the stretch on both sides
    assert float(rp.mean[0, 0]) < theta
    own = m.discover_wavs([one, two], threshold=theta, n_hits=1, min_len=5)   # one list: (0,0) (0,1) (1,1), self pairs banded
    assert len(own) == 3 and torch.equal(own.a_start[1, 0], rp.a_start[0, 0]) and torch.equal(own.b_end[1, 0], rp.b_end[0, 0])
    k = int(own.count[0])
    assert bool((own.b_start[0, :k] - own.a_start[0, :k] >= 5).all())
    after = _model_words(m)
    assert all(torch.equal(_bits(before[k]), _bits(after[k])) for k in before)


def test_refusals_of_the_surface():
    hps, m, _ = _model("vae")
    rows = [torch.zeros(5, dtype=torch.int64, device=DEV)]
    with pytest.raises(L.AewError, match="discrete codes"):
        m.discover_codes(rows, threshold=1.0)
    with pytest.raises(L.AewError, match="discrete codes"):
        m.discover_wavs([torch.zeros(4000, device=DEV)], threshold=1.0)
    with pytest.raises(L.AewError, match="different devices"):
        AL.discover([torch.zeros(3, 4, device=DEV)], [torch.zeros(3, 4)], threshold=1.0)
    with pytest.raises(L.AewError, match="threshold"):
        AL.discover([torch.zeros(3, 4, device=DEV)])


# ---- one plan holding the op, from a captured graph ------------------------------------------------------------------------
def test_a_captured_plan_gives_the_bits_of_the_direct_run():
    A, B = _seqs("normal", 3, LENS, LENS)
    pairs = [(8, 7), (4, 3), (0, 8), (3, 3), (5, 5)]
    x = _Discover(SD.EUCLID, 1.2, _Side(A, "frame"), _Side(B, "chan"), pairs).run()
    direct = x.results()
    p = Plan("discover")
    p.add(L.OP_SEQ_DISCOVER, x.rec, "seq.discover")
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    for rep in range(3):                                                          # capture + first launch, then two replays
        x.refill()
        torch.cuda.synchronize()
        p.run_graph(st)                     # (a capture succeeds only if the op neither allocates nor synchronises)
        got = x.results()
        assert all(got[k].tobytes() == direct[k].tobytes() for k, _ in _Discover.OUTS) and got["bad"] == 0
    assert p._graph is not None
    p.invalidate_graph()
