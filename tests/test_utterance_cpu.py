"""Whole-utterance encoding without a GPU: codes.tile_plan against its plain-loop restatement (tests/utterance_emulator.py)
- every code of every utterance produced exactly once, in order; aew_utterance_locate - compiled from the helpers the
kernels call - against the emulator, and its refusals; the launchers' refusals, which come before any launch and so need
no device; the premise of the whole feature, with the bit-exact yardstick of the GPU encoder (oracle/exact.py): the exact
chain run over a whole utterance gives, frame for frame, the bytes it gives on zero-padded tiles of mel_len frames at hop
s * E; UtteranceCodes and its .npz."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, codes as CD, config, geometry as G
from tests import utterance_emulator as UE
from tests.conftest import GOLDEN

E7, B3, N_MEL = 7, 3, 39


def geometry():
    """(E, s, rf, mel_len) read off the geometry of the small model of tests/test_codes_gpu.py::_model."""
    hps = config.make_hps("vqvae", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64, bn_n_out=16,
                          bn_vq_n_embed=128, n_win_batch=96, n_blocks=2, n_block_layers=4)
    return G.utterance_geometry(G.model_geometry(hps, True, 96))


def test_geometry_states_stride_and_receptive_field():
    E, s, rf, mel_len = geometry()
    assert (s, rf) == G.encoder_stride_rf() == (2, 16) and mel_len == s * (E - 1) + rf and E >= 2
    # the receptive field is what the valid-convolution arithmetic of model_geometry says: rf frames give one code,
    # every s more give one more
    n = rf
    for f, st in zip(G.ENCODER_FILTERS, G.ENCODER_STRIDES):
        n = (n - f) // st + 1
    assert n == 1 and [G.utterance_codes(F, s, rf) for F in (0, rf - 1, rf, rf + s - 1, rf + s, mel_len)] == [0, 0, 1, 1, 2, E]


@pytest.mark.parametrize("E", [E7, geometry()[0]])
def test_tile_plan_produces_every_code_once_in_order(E):
    _, s, rf, _ = geometry()
    mel_len = s * (E - 1) + rf
    cases = UE.case_frames(E, s, rf)
    assert len(cases) == 10 and len(set(cases)) == 10
    frames = UE.mixed_frames(E, s, rf)                                    # the ten, mixed, + one more short utterance
    assert sorted(frames[:10]) == sorted(cases) and len(frames) == 11
    want_off, want_rows, n_rows = UE.tile_plan(frames, E, s, rf, B3)
    p = CD.tile_plan(frames, E, s, rf, B3)
    assert p.mel_len == mel_len and p.n_rows == n_rows and p.offsets.tolist() == want_off and p.n_codes == want_off[-1]
    assert len(p.utt) == len(want_rows) == p.n_batches * B3
    for name in ("utt", "window", "start", "avail", "n_valid", "dst"):
        assert getattr(p, name).tolist() == [r[name] for r in want_rows], name
    # the counts of the ten cases: no code (its offsets repeat), 1, 1, 2, E - 1, E, E, E + 1, 3 E, 4 E - 1
    by_case = [0, 1, 1, 2, E - 1, E, E, E + 1, 3 * E, 4 * E - 1]
    assert np.diff(p.offsets).tolist() == [by_case[i] for i in UE.MIX] + [1]
    u0 = UE.MIX.index(0)
    assert p.offsets[u0] == p.offsets[u0 + 1]
    # every code exactly once, in order: the stored ranges of the live rows, in row order, tile [0, n_codes)
    at = 0
    for k in range(n_rows):
        assert p.dst[k] == at and 1 <= p.n_valid[k] <= E
        u, w = p.utt[k], p.window[k]
        assert p.dst[k] == p.offsets[u] + w * E and p.start[k] == w * s * E
        # a stored code's receptive field lies inside the frames that exist, the first code dropped does not
        last = p.n_valid[k] - 1
        assert last * s + rf <= p.avail[k] <= mel_len
        assert p.n_valid[k] == E or p.n_valid[k] * s + rf > p.avail[k]
        at += p.n_valid[k]
    assert at == p.n_codes
    windows = [int((p.utt[:n_rows] == u).sum()) for u in range(11)]
    assert windows == [[0, 1, 1, 1, 1, 1, 1, 2, 3, 4][i] for i in UE.MIX] + [1]
    assert p.n_valid[p.utt == UE.MIX.index(7)].tolist() == [E, 1]          # the second window holds one code
    # B = 3: windows of one utterance straddle batches, and the last batch has idle rows
    batch_of = np.arange(len(p.utt)) // B3
    assert any(len(set(batch_of[p.utt == u].tolist())) > 1 for u in range(11))
    idle = p.utt[n_rows:]
    assert n_rows == 16 and len(idle) == 2 and (idle == -1).all()
    assert not p.avail[n_rows:].any() and not p.n_valid[n_rows:].any()
    # the records
    bases, n_src = UE.bases_of(frames, N_MEL)
    assert p.table(bases).tobytes() == UE.table(want_rows, frames, bases).tobytes()
    assert p.table(bases).dtype.itemsize == C.sizeof(L.UttRow) == 32


def test_tile_plan_edges():
    _, s, rf, _ = geometry()
    p = CD.tile_plan([], E7, s, rf, 4)
    assert p.n_batches == 0 and p.offsets.tolist() == [0] and len(p.table([])) == 0
    p = CD.tile_plan([0, rf - 1], E7, s, rf, 4)
    assert p.n_batches == 0 and p.offsets.tolist() == [0, 0, 0]
    p = CD.tile_plan([rf], E7, s, rf, 4)
    assert p.n_batches == 1 and p.utt.tolist() == [0, -1, -1, -1] and p.n_valid.tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        CD.tile_plan([-1], E7, s, rf, 4)
    with pytest.raises(ValueError):
        CD.tile_plan([20], E7, s, rf, 0)


def c_locate(rec, n_mel, mel_len, E, n_src, n_dst, i):
    src, avail, nv = C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    row = L.UttRow.from_buffer_copy(rec.tobytes())
    rc = L.load().aew_utterance_locate(C.byref(row), n_mel, mel_len, E, n_src, n_dst, i, C.byref(src), C.byref(avail),
                                       C.byref(nv))
    return None if rc == L.E_ARG else (src.value, avail.value, nv.value) if rc == 0 else rc


def test_locate_agrees_with_the_emulator_on_the_ten_cases():
    _, s, rf, _ = geometry()
    E, n_mel = E7, 5
    mel_len = s * (E - 1) + rf
    frames = UE.mixed_frames(E, s, rf)
    offsets, rows, n_rows = UE.tile_plan(frames, E, s, rf, B3)
    bases, n_src = UE.bases_of(frames, n_mel)
    tbl = UE.table(rows, frames, bases)
    for k in range(len(tbl)):
        for i in range(n_mel * mel_len):
            got = c_locate(tbl[k], n_mel, mel_len, E, n_src, offsets[-1], i)
            assert got is not None and got == UE.locate(tbl[k], n_mel, mel_len, E, n_src, offsets[-1], i), (k, i)
    # every frame of every utterance that has a code is read by some row, and no element outside the buffer is
    seen = set()
    for k in range(n_rows):
        for i in range(n_mel * mel_len):
            so = c_locate(tbl[k], n_mel, mel_len, E, n_src, offsets[-1], i)[0]
            assert -1 <= so < n_src
            seen.add(so)
    need = {bases[u] + c * F + t for u, F in enumerate(frames) if F >= rf for c in range(n_mel)
            for t in range(rf + s * (UE.n_codes(F, s, rf) - 1))}
    assert need <= seen


def _good():
    return np.array([(100, 20, 50, 28, 7, 0)], UE.ROW)[0].copy()


@pytest.mark.parametrize("field,value", [("avail", 29), ("avail", -1), ("n_valid", 8), ("n_valid", -1), ("src", -1),
                                         ("pitch", 27), ("src", 1000 - (4 * 50 + 28) + 1), ("dst", -1), ("dst", 94),
                                         ("pitch", 1 << 30)])
def test_locate_and_the_launchers_refuse_malformed_records(field, value):
    n_mel, mel_len, E, n_src, n_dst = 5, 28, 7, 1000, 100
    rec = _good()
    assert c_locate(rec, n_mel, mel_len, E, n_src, n_dst, 0) == (100, 28, 7)
    assert c_locate(rec, n_mel, mel_len, E, n_src, n_dst, n_mel * mel_len - 1) == (100 + 4 * 50 + 27, 28, 7)
    edge = _good()
    edge["src"], edge["dst"] = 1000 - (4 * 50 + 28), 93                  # the last element / code the buffers hold
    assert c_locate(edge, n_mel, mel_len, E, n_src, n_dst, 0) is not None
    rec[field] = value
    assert UE.locate(rec, n_mel, mel_len, E, n_src, n_dst, 0) is None
    assert c_locate(rec, n_mel, mel_len, E, n_src, n_dst, 0) is None
    # the launchers: aew_run_plan reaches their checks without a device and returns before any launch (made-up device
    # addresses; table_host is real host memory, row 1 of it is the bad one)
    tbl = np.stack([_good(), rec])
    for kind, bad_for in ((L.OP_MEL_TILE, ("avail", "src", "pitch")), (L.OP_CODE_STITCH, ("n_valid", "dst"))):
        if field in bad_for:
            assert run(kind, tbl, first_row=1, B=1) == L.E_ARG
            assert run(kind, tbl, first_row=0, B=2) == L.E_ARG


def run(kind, tbl, **over):
    """One launcher's verdict on a record that is complete but for `over` (never launched: only refusals are asked for)."""
    if kind == L.OP_MEL_TILE:
        rec = L.MelTile()
        rec.mel, rec.n_src, rec.in_mel, rec.n_mel, rec.mel_len = 0x20000, 1000, 0x30000, 5, 28
    else:
        rec = L.CodeStitch()
        rec.ind, rec.min_dist, rec.codes, rec.dist, rec.n_dst, rec.E = 0x20000, 0x30000, 0x40000, 0x50000, 100, 7
    rec.table, rec.table_host, rec.first_row, rec.B = 0x10000, tbl.ctypes.data, 0, 1
    for k, v in over.items():
        setattr(rec, k, v)
    op = L.Op()
    op.kind = kind
    setattr(op.u, L.OP_FIELD[kind], rec)
    fail = C.c_int(-1)
    return L.load().aew_run_plan(C.byref(op), 1, None, C.byref(fail))


def test_launchers_refuse_malformed_descriptors():
    tbl = np.stack([_good(), _good()])
    for kind, nulls in ((L.OP_MEL_TILE, ("table", "table_host", "mel", "in_mel")),
                        (L.OP_CODE_STITCH, ("table", "table_host", "ind", "codes", "min_dist"))):
        for f in nulls:
            assert run(kind, tbl, **{f: None}) == L.E_ARG, (kind, f)
        for f, v in (("B", 0), ("B", -1), ("B", 65536), ("first_row", -1)):
            assert run(kind, tbl, **{f: v}) == L.E_ARG, (kind, f, v)
        assert run(kind, tbl, table=0x10004) == L.E_ALIGN
    assert run(L.OP_MEL_TILE, tbl, n_mel=0) == L.E_ARG and run(L.OP_MEL_TILE, tbl, mel_len=27) == L.E_ARG
    assert run(L.OP_MEL_TILE, tbl, mel=0x20002) == L.E_ALIGN
    assert run(L.OP_CODE_STITCH, tbl, E=6) == L.E_ARG and run(L.OP_CODE_STITCH, tbl, n_dst=26) == L.E_ARG
    assert run(L.OP_CODE_STITCH, tbl, codes=0x40004) == L.E_ALIGN


def test_abi_mirror_of_the_new_records():
    lib = L.load()
    assert lib.aew_sizeof(34) == C.sizeof(L.UttRow) == np.dtype(L.UTT_ROW_DTYPE).itemsize == UE.ROW.itemsize == 32
    assert lib.aew_sizeof(35) == C.sizeof(L.MelTile) and lib.aew_sizeof(36) == C.sizeof(L.CodeStitch)
    assert lib.aew_sizeof(33) == -1 and lib.aew_abi_version() == 28              # (33 is left unused, like 24 and 26)
    assert max(C.sizeof(L.MelTile), C.sizeof(L.CodeStitch)) <= C.sizeof(L.GemmNT)       # sizeof(aew_op_t) did not move
    assert (L.OP_MEL_TILE, L.OP_CODE_STITCH) == (L.OP_EVAL_GROUPS + 1, L.OP_EVAL_GROUPS + 2)
    assert L.OP_FIELD[L.OP_MEL_TILE] == "mtile" and L.OP_FIELD[L.OP_CODE_STITCH] == "cstitch"
    assert "aew_utterance_locate" in L.EXPORTS
    assert [n for n, _ in L.UTT_ROW_DTYPE] == [n for n, _ in L.UttRow._fields_] == list(UE.ROW.names)


# ---- the premise: the exact chain over a whole utterance == over zero-padded tiles ------------------------------------
def _chain(width, d=16, K=128, seed=11):
    sys.path.insert(0, GOLDEN)
    from weights import np_weights
    shapes = {}
    for i, f in enumerate(G.ENCODER_FILTERS):
        shapes[f"encoder.net.{i}.conv.weight"] = (width, N_MEL if i == 0 else width, f)
        shapes[f"encoder.net.{i}.conv.bias"] = (width,)
    shapes["bottleneck.linear.weight"] = (d, width, 1)
    wts = np_weights(shapes, seed)
    emb = (np.random.RandomState(seed + 1).standard_normal((K, d)) * 0.7).astype(np.float32)
    return wts, emb


def _exact(wts, emb, mel_cl):
    """(ze (B, N, d), ind (B * N,), dist (B * N,)) of encoder_cl -> linear_cl -> vq_nearest on channels-last mel."""
    from oracle import exact
    ze = exact.linear_cl(exact.encoder_cl(wts, "encoder.", mel_cl), wts["bottleneck.linear.weight"])
    ind, dist, _ = exact.vq_nearest(ze.reshape(-1, ze.shape[2]), emb, "scaled_l2")
    return ze, ind, dist


@pytest.mark.parametrize("width", [64, 768])                                  # (768: the exact GEMMs' split-K width)
def test_whole_utterance_equals_its_tiles_in_the_exact_chain(width):
    _, s, rf, _ = geometry()
    E = E7
    mel_len = s * (E - 1) + rf
    wts, emb = _chain(width)
    rs = np.random.RandomState(width)
    done = []
    for F in UE.case_frames(E, s, rf):
        mel = rs.standard_normal((N_MEL, F)).astype(np.float32)
        wins, keep = UE.cut_windows(mel, E, s, rf)
        N = UE.n_codes(F, s, rf)
        assert wins.shape == (-(-N // E), N_MEL, mel_len) and sum(keep) == N
        done.append(F)
        if N == 0:                                                             # below the receptive field: no window at all
            assert F == rf - 1 and not keep
            continue
        ze_w, ind_w, dist_w = _exact(wts, emb, np.ascontiguousarray(mel.T)[None])
        ze_t, ind_t, dist_t = _exact(wts, emb, np.ascontiguousarray(wins.transpose(0, 2, 1)))
        assert ze_w.shape == (1, N, 16) and ze_t.shape == (len(keep), E, 16)
        ze_cat = np.concatenate([ze_t[w, :k] for w, k in enumerate(keep)])
        ind_cat = np.concatenate([ind_t.reshape(-1, E)[w, :k] for w, k in enumerate(keep)])
        dist_cat = np.concatenate([dist_t.reshape(-1, E)[w, :k] for w, k in enumerate(keep)])
        assert ze_cat.tobytes() == ze_w[0].tobytes(), F
        assert np.array_equal(ind_cat, ind_w) and dist_cat.tobytes() == dist_w.tobytes(), F
    assert done == UE.case_frames(E, s, rf) and len(done) == 10


# ---- UtteranceCodes ---------------------------------------------------------------------------------------------------
def _codes(with_all=True):
    rs = np.random.RandomState(3)
    offsets = [0, 0, 4, 5, 12]
    kw = dict(dist=torch.from_numpy(rs.rand(12).astype(np.float32)), voice=torch.tensor([3, 0, 7, 7]),
              names=["a/1.wav", "b/2.wav", "ü.flac", ""]) if with_all else {}
    return CD.UtteranceCodes(torch.from_numpy(rs.randint(0, 128, 12).astype(np.int64)), torch.tensor(offsets), **kw)


def test_utterance_codes_rows_and_padding():
    uc = _codes()
    assert len(uc) == 4 and [uc.row(u).numel() for u in range(4)] == [0, 4, 1, 7]
    assert torch.equal(uc.row(-1), uc.codes[5:]) and uc.row(1).data_ptr() == uc.codes.data_ptr()
    with pytest.raises(IndexError):
        uc.row(4)
    pad = uc.padded()
    assert pad.shape == (4, 7) and pad.dtype == torch.int64 and (pad[0] == -1).all()
    for u in range(4):
        n = uc.row(u).numel()
        assert torch.equal(pad[u, :n], uc.row(u)) and (pad[u, n:] == -1).all()
    assert (uc.padded(fill=128)[2, 1:] == 128).all()
    with pytest.raises(L.AewError):
        CD.UtteranceCodes(uc.codes, torch.tensor([0, 11]))
    with pytest.raises(L.AewError):
        CD.UtteranceCodes(uc.codes, uc.offsets, voice=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(L.AewError):
        CD.UtteranceCodes(uc.codes, uc.offsets, names=["x"])
    empty = CD.UtteranceCodes(torch.zeros(0, dtype=torch.int64), torch.tensor([0]))
    assert len(empty) == 0 and empty.padded().shape == (0, 0)


@pytest.mark.parametrize("with_all", [True, False])
def test_utterance_codes_npz_round_trip(tmp_path, with_all):
    uc = _codes(with_all)
    path = tmp_path / "codes.npz"
    uc.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == (["codes", "dist", "names", "offsets", "voice"] if with_all else ["codes", "offsets"])
    back = CD.UtteranceCodes.load(path)
    assert torch.equal(back.codes, uc.codes) and torch.equal(back.offsets, uc.offsets) and back.codes.dtype == torch.int64
    if with_all:
        assert back.dist.numpy().tobytes() == uc.dist.numpy().tobytes() and torch.equal(back.voice, uc.voice)
        assert back.names == uc.names
    else:
        assert back.dist is None and back.voice is None and back.names is None
