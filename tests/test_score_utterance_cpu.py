"""Whole-utterance scoring, the host side: geometry.scoring_geometry and codes.score_tile_plan against their restatement
(tests/score_utterance_emulator.py), the owned outputs partitioning every utterance's scored samples, their read sets
inside real rows and real codes, the numpy emulators of the three ops tiling a toy causal decoder exactly, the ABI
additions, and the launchers' refusals (which come before any launch, so they run without a GPU)."""
import ctypes as C

import numpy as np
import pytest

from ae_wavenet_amd import _lib as L, codes as CD, config, geometry as G
from tests import cond_utterance_emulator as CE, score_utterance_emulator as SE
from tests.test_cond_utterance_cpu import SMALL, _geom


# ---- 1. geometry -------------------------------------------------------------------------------------------------------
def test_scoring_geometry_of_the_test_model_and_of_the_reference():
    hps, g = _geom(1000, **SMALL)
    sg = G.scoring_geometry(g)
    assert (sg.E, sg.S, sg.T, sg.rf, sg.r0, sg.p, sg.h_s, sg.o) == (11, 320, 1030, 30, 0, 0, 3, 2235) == sg.plan_args()[:8]
    assert sg.h_s == G.conditioning_geometry(g).h == 3                   # (in the small model both hops are 3)
    assert (sg.p, sg.r0, sg.h_s) == SE.hop(sg.S, sg.T, sg.rf, g.trim_ups_out[0])
    assert [sg.L(n) for n in CE.CASES] == [0, 68, 708, 1028, 1348, 1668, 3268]
    # the window model the tiling rests on: T = n_win + rf, the target of output u is decoder-input sample u + rf + 1
    assert g.dec_in_len == g.n_win + g.rf and g.wav_out_off == g.trim_dec_in[0] + g.rf
    # the reference geometry at n_win = 5000: the last output carries no loss, so the scoring hop is NOT the conditioning hop
    hps, g = _geom(5000)
    sg, cg = G.scoring_geometry(g), G.conditioning_geometry(g)
    assert (sg.E, sg.T, sg.rf, sg.r0, sg.p, sg.o) == (29, 7046, 2046, 0, 0, 2235)
    assert cg.h == 22 and sg.h_s == (5000 - 1) // 320 == 15 and sg.h_s != cg.h
    assert sg.r0 + sg.h_s * sg.S <= g.n_win - 1 < sg.r0 + (sg.h_s + 1) * sg.S


def test_a_window_too_small_to_tile_is_refused_with_the_size_that_works():
    with pytest.raises(L.AewError, match="n_win_batch >= 321"):
        G.scoring_geometry(_geom(320, **SMALL)[1])                      # (the conditioning tiles there: h = 1)
    assert G.conditioning_geometry(_geom(320, **SMALL)[1]).h == 1
    assert G.scoring_geometry(_geom(321, **SMALL)[1]).h_s == 1          # and that size is the smallest
    with pytest.raises(L.AewError, match="n_win_batch"):
        G.scoring_geometry(_geom(96, **SMALL)[1])                       # (refused by the conditioning geometry already)
    L_of = lambda n: CE.length(n, CE.REF_FILTERS, CE.REF_STRIDES)
    with pytest.raises(ValueError):
        CD.score_tile_plan([17], [9000], (11, 320, 350, 30, 0, 0, 1, 2235, L_of), 1)     # 350 - 30 - 1 < 320
    with pytest.raises(ValueError):
        CD.score_tile_plan([17], [9000], (11, 320, 1030, 30, 0, 0, 4, 2235, L_of), 1)    # a hop the window cannot hold
    with pytest.raises(ValueError):
        CD.score_tile_plan([17, 3], [9000], (11, 320, 1030, 30, 0, 0, 3, 2235, L_of), 1)


# ---- 2. the tile plan --------------------------------------------------------------------------------------------------
# (E, S, T, rf, trim0, o, filters, strides, L): the synthetic odd geometry of the conditioning op tests (L(n) = 5 n - 9 is
# stated, not derived from a filter set: p = 1, r0 = 2, h = 3; rf = 4 gives 14 outputs and h_s = (13 - 2) // 5 = 2), a
# real filter set with trim0 != 0, the test model, the reference at n_win = 5000
SYN = (7, 5, 18, 4, 3, 6, None, None, lambda n: max(5 * n - 9, 0))
ODD = (9, 6, 25, 5, 4, 3, (4, 6), (2, 3), None)
SMALL_G = (11, 320, 1030, 30, 0, 2235, CE.REF_FILTERS, CE.REF_STRIDES, None)
REF_G = (29, 320, 7046, 2046, 0, 2235, CE.REF_FILTERS, CE.REF_STRIDES, None)


def _lengths(geom):
    """(n_codes, wav_lens) that meet every edge: n_u = 0, rf + 1 (nothing scored), rf + 2 (one sample), one hop exactly,
    one hop plus 1, several hops, a waveform shorter than o + L(N), a waveform shorter than o."""
    E, S, T, rf, trim0, o, filters, strides, L_of = geom
    L_of = L_of or (lambda n: CE.length(n, filters, strides))
    p, r0, h_s = SE.hop(S, T, rf, trim0)
    big = next(n for n in range(1, 10000) if L_of(n) >= 3 * h_s * S + rf + 9)
    cases = [(0, o + 50), (1, o + 50), (big, o), (big, o - 1 if o else 0), (big, o + rf + 1), (big, o + rf + 2),
             (big, o + rf + 1 + h_s * S), (big, o + rf + 2 + h_s * S), (big, o + rf + 1 + 2 * h_s * S - 1),
             (big, o + L_of(big) + 100), (big, o + L_of(big) - 7), (big + 3, o + L_of(big + 3))]
    first = next(n for n in range(1, 10000) if L_of(n) > 0)
    cases += [(first, o + 10 ** 6), (first + 1, o + 10 ** 6), (first + 2, o + 10 ** 6)]
    return [c[0] for c in cases], [c[1] for c in cases], L_of, (p, r0, h_s)


@pytest.mark.parametrize("geom", [SYN, ODD, SMALL_G, REF_G], ids=["synthetic", "odd", "test-model", "reference"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_owned_outputs_partition_the_scored_samples_and_read_real_rows_only(geom, B):
    E, S, T, rf, trim0, o, filters, strides, _ = geom
    n_codes, wav_lens, L_of, (p, r0, h_s) = _lengths(geom)
    if geom is SYN:
        assert h_s == 2 and h_s != CE.hop(S, T, trim0)[2] == 3
    if geom is REF_G:
        assert h_s == 15 and h_s != CE.hop(S, T, trim0)[2] == 22
    w = T - rf
    plan = CD.score_tile_plan(n_codes, wav_lens, (E, S, T, rf, r0, p, h_s, o, L_of), B)
    n_us, n_sc, offsets, rows, n_rows = SE.tile_plan(n_codes, wav_lens, E, S, T, rf, trim0, o, B, L_of)
    assert plan.n_u.tolist() == n_us and plan.n_scored.tolist() == n_sc and plan.offsets.tolist() == offsets
    assert plan.n_rows == n_rows and len(plan.utt) == len(rows) and len(rows) % B == 0 and plan.n_batches * B == len(rows)
    assert plan.n_total == offsets[-1] == sum(n_sc)
    for name, arr in (("utt", plan.utt), ("window", plan.window), ("start", plan.start), ("lo", plan.lo), ("hi", plan.hi),
                      ("wav0", plan.wav0), ("src", plan.src), ("n_out", plan.n_out), ("dst", plan.dst)):
        assert arr.tolist() == [r[name] for r in rows], name
    assert 0 in n_us and rf + 1 in n_us and rf + 2 in n_us and rf + 1 + h_s * S in n_us and rf + 2 + h_s * S in n_us
    assert sorted(set(n_sc))[:2] == [0, 1] and h_s * S in n_sc and h_s * S + 1 in n_sc
    code_bases = np.concatenate([[0], np.cumsum(n_codes)])[:-1]
    wav_bases = np.concatenate([[0], np.cumsum(wav_lens)])[:-1]
    voices = np.arange(len(n_codes)) % 7
    tbl = plan.table(code_bases, wav_bases, voices)
    assert tbl.dtype.itemsize == 64 and tbl.tobytes() == SE.table(rows, code_bases, wav_bases, wav_lens, voices).tobytes()
    # idle rows only pad the last batch
    idle = np.flatnonzero(tbl["utt"] < 0)
    assert len(idle) < B and (len(idle) == 0 or idle.tolist() == list(range(len(tbl) - len(idle), len(tbl))))
    count = np.zeros(offsets[-1], np.int64)
    target = np.full(offsets[-1], -1, np.int64)
    for r in tbl:
        if r["utt"] < 0:
            assert not any(r[k] for k in ("n_out", "hi", "lo", "dst"))
            continue
        u, j = int(r["utt"]), int(r["wav0"] - o + r0) // (h_s * S)
        a_j = j * h_s * S - r0                                           # the utterance position of the window's cond row 0
        assert r["n_out"] > 0 and r0 <= r["src"] and r["src"] + r["n_out"] <= r0 + h_s * S <= w - 1    # u = w - 1 has no loss
        assert offsets[u] <= r["dst"] and r["dst"] + r["n_out"] <= offsets[u + 1]
        assert 0 <= r["lo"] <= r["hi"] <= E and r["voice"] == voices[u]
        assert code_bases[u] <= r["code0"] + r["lo"] and r["code0"] + r["hi"] <= code_bases[u] + n_codes[u]
        assert r["wav_base"] == wav_bases[u] and r["wav_len"] == wav_lens[u] and r["wav0"] == o + a_j
        start = int(r["code0"] - code_bases[u])
        assert start == j * h_s - p
        for i in (0, int(r["n_out"]) - 1):                              # the first and the last owned output bound the rest
            uo = int(r["src"]) + i
            q_t = a_j + uo + rf + 1
            assert rf + 1 <= q_t < n_us[u]
            # its read set: decoder-input rows and cond rows [uo, uo + rf] of the window = positions [q_t - rf - 1, q_t - 1]
            assert 0 <= q_t - rf - 1 and q_t - 1 < n_us[u] and uo + rf + 1 < T
            assert 0 <= o + q_t - rf - 1 and o + q_t < wav_lens[u]      # ... real samples, the target included
            if filters is not None:                                     # ... and real codes, all inside the window
                for q in (q_t - rf - 1, q_t - 1):
                    c_lo, c_hi = SE.code_span(q, filters, strides)
                    assert 0 <= c_lo and c_hi < n_codes[u]
                    assert r["lo"] <= c_lo - start and c_hi - start < r["hi"]
                    w_lo, w_hi = SE.code_span(q - a_j + trim0, filters, strides)     # the same row, in window coordinates
                    assert (w_lo, w_hi) == (c_lo - start, c_hi - start)
        d = int(r["dst"])
        count[d:d + r["n_out"]] += 1
        target[d:d + r["n_out"]] = a_j + r["src"] + np.arange(r["n_out"]) + rf + 1
    assert (count == 1).all()                                           # every scored sample exactly once
    for u in range(len(n_codes)):                                       # ... in order: element i of row u is position rf + 1 + i
        assert target[offsets[u]:offsets[u + 1]].tolist() == list(range(rf + 1, n_us[u]))
    empty = CD.score_tile_plan([], [], (E, S, T, rf, r0, p, h_s, o, L_of), 4)
    assert empty.n_rows == 0 and len(empty.utt) == 0 and empty.n_total == 0 and empty.offsets.tolist() == [0]


def test_code_span_is_what_the_chain_reads():
    """The emulator's closed form against the chain itself: changing a code inside the span changes the row, changing
    the codes next to it does not."""
    filters, strides = (4, 6), (2, 3)
    wts = CE.small_weights(filters, 16, 3, 4, seed=3)
    wts["emb"] = np.arange(16 * 3, dtype=np.float64).reshape(16, 3) + 1.0      # (distinct rows: every code matters)
    wts["lc"] = np.ones_like(wts["lc"])
    wts["ups"] = [np.ones_like(W) for W in wts["ups"]]
    codes = np.arange(1, 13) % 16
    whole = CE.chain(codes, wts, filters, strides)
    for q in range(whole.shape[0]):
        c_lo, c_hi = SE.code_span(q, filters, strides)
        assert 0 <= c_lo <= c_hi < len(codes)
        for c in range(len(codes)):
            other = codes.copy()
            other[c] = (other[c] + 5) % 16
            changed = not (CE.chain(other, wts, filters, strides)[q] == whole[q]).all()
            assert changed == (c_lo <= c <= c_hi), (q, c)


# ---- 3. the tiling is exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [ODD, (9, 6, 26, 3, 7, 0, (4, 6), (2, 3), None), (11, 320, 1030, 30, 0, 2235, CE.REF_FILTERS, CE.REF_STRIDES, None)],
                         ids=["odd", "odd-p2", "test-model"])
def test_tiles_stitched_equal_one_run_over_the_whole_sequence(geom):
    E, S, T, rf, trim0, o, filters, strides, _ = geom
    K, d, Cc = 16, 3, 2
    wts = CE.small_weights(filters, K, d, Cc, seed=E + trim0)
    rs = np.random.RandomState(T)
    L_of = lambda n: CE.length(n, filters, strides)
    p, r0, h_s = SE.hop(S, T, rf, trim0)
    big = 17 if S == 320 else next(n for n in range(1, 1000) if L_of(n) >= 4 * h_s * S + rf + 5)
    n_codes = [0, 1, big, big, big, big - 2, next(n for n in range(1, 1000) if L_of(n) > rf + 1)]
    wav_lens = [o + 9, o + 9, o + L_of(big) + 5, o + rf + 2 + h_s * S, o - 0 if o else 0, o + L_of(big - 2) - 3, o + 10 ** 4]
    codes = [rs.randint(1, K, n) for n in n_codes]                       # (code 0 is the pad code: never a real one)
    wavs = [rs.randint(0, 256, n).astype(np.float32) for n in wav_lens]
    got, count = SE.toy_tiled(codes, wavs, wts, filters, strides, E, S, T, rf, trim0, o, B=3)
    n_windows = 0
    for u, (c, x) in enumerate(zip(codes, wavs)):
        whole = SE.toy_whole(c, x, wts, filters, strides, rf, o)
        assert whole.shape == got[u].shape == (max(min(L_of(len(c)), len(x) - o) - rf - 1, 0),)
        assert (count[u] == 1).all()
        assert (got[u] == whole).all(), u                                 # exact sums: ==, not a tolerance
        assert np.abs(whole).max(initial=0) < 2 ** 50
        n_windows += -(-len(whole) // (h_s * S))
    assert n_windows > len(codes) and any(len(g) > 2 * h_s * S for g in got)      # several windows were stitched
    # neither the pad code nor the zero code behind an utterance matters: other values change no owned output
    wts2 = dict(wts, emb=wts["emb"].copy())
    wts2["emb"][0] += 1.0
    again, _ = SE.toy_tiled(codes, wavs, wts2, filters, strides, E, S, T, rf, trim0, o, B=2, zero=3.0)
    assert all((a == b).all() for a, b in zip(again, got))


def test_wav_tile_emulator_counts_what_it_replaces():
    tbl = np.zeros(2, SE.ROW)
    tbl["utt"] = [0, -1]
    tbl[0] = (1, 2, 6, -2, 0, 0, 1, 3, 4, 0, 0)
    codes = np.array([9, 5, 99, 7, 8], np.int64)
    wavs = np.array([1, 1, 0, 255, 256, -1, np.nan, 1e9, 7, 7], np.float32)
    wav, ind, voice, bad_c, bad_w = SE.wav_tile(tbl, 0, 2, codes, wavs, E=4, K=16, T=10, n_quant=256, zero=128.0)
    assert wav[0].tolist() == [128, 128, 0, 255, 128, 128, 128, 128, 128, 128] and (wav[1] == 128).all()
    assert ind.tolist() == [[0, 0, 7, 0], [0, 0, 0, 0]] and voice.tolist() == [4, 0] and (bad_c, bad_w) == (1, 4)


def test_reduce_emulator_follows_the_fixed_order():
    rs = np.random.RandomState(0)
    x = (rs.standard_normal(5000) * 3).astype(np.float32)
    s = np.zeros(1024)
    for i, v in enumerate(x):                                            # thread i % 1024 adds its elements ascending
        s[i % 1024] += float(v)
    o = 512
    while o:
        for t in range(o):
            s[t] += s[t + o]
        o >>= 1
    assert SE.tree_sum(x) == s[0]
    hit = (rs.rand(5000) < 0.3).astype(np.uint8)
    acc, out = SE.score_reduce([0, 0, 3000, 5000], x, np.abs(x), hit)
    assert acc[0].tolist() == [0, 0, 0, 0] and out[0].tolist() == [0, 0, 0, 0]
    assert acc[1, 0] == 3000 and acc[1, 3] == hit[:3000].sum() and acc[2, 1] == SE.tree_sum(x[3000:])
    assert out[1, 0] == np.float32(acc[1, 1] / 3000) and out[1, 2] == np.float32(hit[:3000].sum() / 3000)
    assert out[1, 1] == np.float32(acc[1, 1] / 3000 / np.log(2.0)) and out[2, 3] == np.float32(acc[2, 2] / 2000)


# ---- 4. the ABI ----------------------------------------------------------------------------------------------------------
def test_abi_additions_are_appended_and_mirrored():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert (L.OP_WAV_TILE, L.OP_NLL_STITCH, L.OP_SCORE_REDUCE) == (L.OP_COND_STITCH + 1, L.OP_COND_STITCH + 2, L.OP_COND_STITCH + 3)
    for which, cls in ((42, L.ScoreRow), (43, L.WavTile), (44, L.NllStitch), (45, L.ScoreReduce)):
        assert lib.aew_sizeof(which) == C.sizeof(cls)
    assert lib.aew_sizeof(42) == np.dtype(L.SCORE_ROW_DTYPE).itemsize == SE.ROW.itemsize == 64
    assert np.dtype(L.SCORE_ROW_DTYPE) == SE.ROW
    for name, _ in L.ScoreRow._fields_:                                  # the numpy record and the ctypes one agree field by field
        assert np.dtype(L.SCORE_ROW_DTYPE).fields[name][1] == getattr(L.ScoreRow, name).offset
    assert lib.aew_sizeof(40) == -1 and lib.aew_sizeof(41) == C.sizeof(L.DrawRec) and lib.aew_sizeof(46) == -1
    assert lib.aew_sizeof(0) == C.sizeof(L.Op) == 1656                   # the op record did not grow
    assert max(C.sizeof(c) for c in (L.WavTile, L.NllStitch, L.ScoreReduce)) <= C.sizeof(L.GemmNT)


# ---- 5. the launchers refuse before any launch (no GPU needed) --------------------------------------------------------------
def _rc(kind, rec):
    op = L.Op()
    op.kind = kind
    setattr(op.u, L.OP_FIELD[kind], rec)
    fail = C.c_int(-1)
    return L.load().aew_run_plan(C.byref(op), 1, None, C.byref(fail))


def _aligned(n_bytes):
    raw = np.zeros(n_bytes + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n_bytes]


def test_launchers_refuse_malformed_calls_on_the_host():
    tbl_b = _aligned(64 * 2)
    tbl = tbl_b.view(SE.ROW)
    tbl["utt"] = -1
    buf = _aligned(4096)
    ptr = buf.ctypes.data

    def wav_tile(**over):
        wt = L.WavTile()
        wt.table = wt.table_host = tbl_b.ctypes.data
        wt.first_row, wt.B, wt.codes, wt.n_codes, wt.wavs, wt.n_wav = 0, 2, ptr, 8, ptr, 8
        wt.ind, wt.in_voice, wt.wav, wt.bad_codes, wt.bad_wav = ptr, ptr, ptr, ptr, ptr
        wt.wav_pitch, wt.wav_off, wt.T, wt.n_quant, wt.E, wt.K, wt.n_voice, wt.zero = 64, 8, 18, 256, 7, 16, 5, 128.0
        for k, v in over.items():
            setattr(wt, k, v)
        return _rc(L.OP_WAV_TILE, wt)

    for over in (dict(table=None), dict(table_host=None), dict(codes=None), dict(wavs=None), dict(ind=None), dict(wav=None),
                 dict(bad_wav=None), dict(bad_codes=None), dict(B=0), dict(first_row=-1), dict(E=0), dict(K=0), dict(T=0),
                 dict(n_quant=0), dict(wav_off=-1), dict(wav_off=47), dict(zero=256.0), dict(zero=-1.0), dict(n_wav=-1)):
        assert wav_tile(**over) == L.E_ARG, over
    assert wav_tile(wav=ptr + 4) == L.E_ALIGN and wav_tile(bad_wav=ptr + 2) == L.E_ALIGN and wav_tile(table=tbl_b.ctypes.data + 8) == L.E_ALIGN
    good = (0, 0, 8, -3, 0, 0, 0, 7, 4, 2, 10)
    for field, value in (("hi", 8), ("lo", -1), ("code0", 2), ("voice", 5), ("wav_len", 9), ("wav_base", 1), ("wav_len", -1),
                         ("wav0", 1 << 40)):
        tbl[0] = good
        tbl[field][0] = value
        assert wav_tile() == L.E_ARG, field
    tbl[0] = good

    def stitch(**over):
        ns = L.NllStitch()
        ns.table = ns.table_host = tbl_b.ctypes.data
        ns.first_row, ns.B, ns.nll, ns.ptgt, ns.amax, ns.wav = 0, 2, ptr, ptr, ptr, ptr
        ns.dst_nll, ns.dst_ptgt, ns.dst_hit, ns.n_dst = ptr, ptr, ptr, 10
        ns.wav_pitch, ns.tgt_off, ns.w = 64, 12, 14
        for k, v in over.items():
            setattr(ns, k, v)
        return _rc(L.OP_NLL_STITCH, ns)

    for over in (dict(nll=None), dict(dst_nll=None), dict(ptgt=None), dict(wav=None), dict(amax=None), dict(w=1), dict(n_dst=9),
                 dict(tgt_off=51), dict(tgt_off=-1), dict(amax=None, logits=ptr, n_quant=256, pitch=255), dict(B=0)):
        assert stitch(**over) == L.E_ARG, over
    assert stitch(dst_nll=ptr + 2) == L.E_ALIGN
    for field, value in (("src", 12), ("n_out", 14), ("n_out", -1), ("src", -1), ("dst", 1), ("dst", -1)):
        tbl[0] = good
        tbl[field][0] = value
        assert stitch() == L.E_ARG, field
    tbl[0] = good
    offs = _aligned(8 * 4).view(np.int64)

    def reduce(o, **over):
        offs[:] = o
        sr = L.ScoreReduce()
        sr.offsets = sr.offsets_host = offs.ctypes.data
        sr.nll, sr.ptgt, sr.hit, sr.n_src, sr.acc, sr.out, sr.U = ptr, ptr, ptr, 100, ptr, ptr, 3
        for k, v in over.items():
            setattr(sr, k, v)
        return _rc(L.OP_SCORE_REDUCE, sr)

    for o, over in (([0, 10, 9, 100], {}), ([-1, 0, 0, 0], {}), ([0, 0, 0, 101], {}), ([0, 1, 2, 3], dict(U=0)),
                    ([0, 1, 2, 3], dict(acc=None)), ([0, 1, 2, 3], dict(offsets_host=None)), ([0, 1, 2, 3], dict(n_src=2))):
        assert reduce(o, **over) == L.E_ARG, (o, over)
    assert reduce([0, 1, 2, 3], acc=ptr + 4) == L.E_ALIGN
