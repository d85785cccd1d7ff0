"""Whole-utterance encoding on the device: AEW_OP_MEL_TILE and AEW_OP_CODE_STITCH alone, byte for byte against their
numpy restatements (tests/utterance_emulator.py) with canaries behind every output and NaN around every source row;
model.encode_utterances() against model.encode() on hand-cut, hand-zero-padded windows and against the bit-exact oracle
run over the whole mel; encode_wavs() / encode_corpus(); one batch replayed from a captured graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, codes as CD, corpus as CP, geometry as G
from ae_wavenet_amd.mfcc import DeviceMfcc
from tests import utterance_emulator as UE
from tests.test_codes_gpu import _bits, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
B3 = 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(kind, rec):
    CD._run(kind, rec, "utterance op", torch.device(DEV))


def _pinned(tbl):
    host = torch.empty(tbl.nbytes, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = tbl.view(np.uint8).reshape(-1)
    return host


# ---- the two ops alone ------------------------------------------------------------------------------------------------
def _ragged_with_nan(frames, n_mel, gap, seed):
    """A source buffer in which every channel row of every utterance is followed (and the first preceded) by `gap`
    NaNs: (buffer, bases, pitches).  A read outside the frames a record names returns NaN."""
    rs = np.random.RandomState(seed)
    parts, bases, at = [np.full(gap, np.nan, np.float32)], [], gap
    for F in frames:
        bases.append(at)
        for c in range(n_mel):
            row = rs.standard_normal(F).astype(np.float32)
            if F:
                row[0] = np.float32(-0.0)                                    # bytes, not values
            parts += [row, np.full(gap, np.nan, np.float32)]
        at += n_mel * (F + gap)
    return np.concatenate(parts), bases, [F + gap for F in frames]


@pytest.mark.parametrize("n_mel,E,shift", [(5, 7, 0), (39, 7, 0), (3, 7, 0), (5, 7, 1), (6, 4, 0), (3, 4, 0)])
def test_mel_tile_and_code_stitch_equal_the_emulator_byte_for_byte(n_mel, E, shift):
    """(5, 7): in_mel rows of 140 floats - 16-byte stores, source rows at every alignment; (39, 7): the product's channel
    count; (3, 7): another pitch parity of the source rows; shift 1: in_mel only 4-byte aligned - the element path;
    (6, 4): mel_len 22, rows of 132 floats whose quads straddle channel seams; (3, 4): rows of 66 floats, no multiple of
    4 - the element path again."""
    s, rf = G.encoder_stride_rf()
    mel_len = s * (E - 1) + rf
    frames = UE.mixed_frames(E, s, rf)
    offsets, rows, n_rows = UE.tile_plan(frames, E, s, rf, B3)
    gap = 2 if n_mel == 3 else 3
    src, bases, pitches = _ragged_with_nan(frames, n_mel, gap, 7 + n_mel)
    tbl = UE.table(rows, frames, bases)
    for k, r in enumerate(rows):
        if r["utt"] >= 0:
            tbl["pitch"][k] = pitches[r["utt"]]
    n_src, n_dst, R = len(src), offsets[-1], len(rows)
    mel_d, tbl_d, tbl_h = _dev(src), _dev(tbl.view(np.uint8).reshape(-1)), _pinned(tbl)
    row_n = n_mel * mel_len
    in_mel = torch.full((shift + B3 * row_n + CANARY,), -7.0, dtype=torch.float32, device=DEV)
    rs = np.random.RandomState(E)
    codes = torch.full((n_dst + CANARY,), -9, dtype=torch.int64, device=DEV)
    dist = torch.full((n_dst + CANARY,), -9.0, dtype=torch.float32, device=DEV)
    want_codes, want_dist = np.full(n_dst, -9, np.int64), np.full(n_dst, -9.0, np.float32)
    saw_idle = 0
    for first in range(0, R, B3):
        mt = L.MelTile()
        mt.table, mt.table_host, mt.first_row, mt.B = tbl_d.data_ptr(), tbl_h.data_ptr(), first, B3
        mt.mel, mt.n_src, mt.in_mel, mt.n_mel, mt.mel_len = mel_d.data_ptr(), n_src, in_mel.data_ptr() + 4 * shift, n_mel, mel_len
        in_mel.fill_(-7.0)
        _run(L.OP_MEL_TILE, mt)
        got = in_mel.cpu().numpy()
        want = UE.mel_tile(tbl, first, B3, src, n_mel, mel_len)
        assert not np.isnan(want).any()
        assert got[shift:shift + B3 * row_n].tobytes() == want.tobytes(), first
        assert (got[:shift] == -7.0).all() and (got[shift + B3 * row_n:] == -7.0).all(), "canary around in_mel"
        for b in range(B3):                                                   # zero BITS behind the frames, idle rows all zero
            a = int(tbl["avail"][first + b])
            tile = got[shift + b * row_n:shift + (b + 1) * row_n].reshape(n_mel, mel_len)
            assert not tile[:, a:].view(np.uint32).any()
            saw_idle += a == 0
        ind = rs.randint(0, 1 << 40, B3 * E).astype(np.int64)
        md = rs.rand(B3 * E).astype(np.float32)
        ind_d, md_d = _dev(ind), _dev(md)
        cs = L.CodeStitch()
        cs.table, cs.table_host, cs.first_row, cs.B = tbl_d.data_ptr(), tbl_h.data_ptr(), first, B3
        cs.ind, cs.min_dist, cs.codes, cs.dist, cs.n_dst, cs.E = ind_d.data_ptr(), md_d.data_ptr(), codes.data_ptr(), dist.data_ptr(), n_dst, E
        _run(L.OP_CODE_STITCH, cs)
        UE.code_stitch(tbl, first, B3, ind, md, want_codes, want_dist, E)
        gc, gd = codes.cpu().numpy(), dist.cpu().numpy()
        assert gc[:n_dst].tobytes() == want_codes.tobytes() and gd[:n_dst].tobytes() == want_dist.tobytes(), first
        assert (gc[n_dst:] == -9).all() and (gd[n_dst:] == -9.0).all(), "canary behind the ragged outputs"
    assert saw_idle == 2 and not (want_codes == -9).any()                     # every code was stored, the idle rows ran
    # without the distance output: codes only, dist untouched
    dist.fill_(-9.0)
    cs.dist, cs.first_row = None, 0
    _run(L.OP_CODE_STITCH, cs)
    assert (dist == -9.0).all()


def test_malformed_records_are_refused_with_nothing_written():
    n_mel, mel_len, E = 5, 28, 7
    good = np.array([(0, 0, 50, 28, 7, 0)] * 2, UE.ROW)
    mel = torch.zeros(n_mel * 50, device=DEV)
    in_mel = torch.full((2 * n_mel * mel_len,), -7.0, device=DEV)
    ind, md = torch.zeros(2 * E, dtype=torch.int64, device=DEV), torch.zeros(2 * E, device=DEV)
    codes, dist = torch.full((14,), -9, dtype=torch.int64, device=DEV), torch.full((14,), -9.0, device=DEV)

    def ops(tbl):
        d, h = _dev(tbl.view(np.uint8).reshape(-1)), _pinned(tbl)
        mt, cs = L.MelTile(), L.CodeStitch()
        mt.table, mt.table_host, mt.first_row, mt.B = d.data_ptr(), h.data_ptr(), 0, 2
        mt.mel, mt.n_src, mt.in_mel, mt.n_mel, mt.mel_len = mel.data_ptr(), mel.numel(), in_mel.data_ptr(), n_mel, mel_len
        cs.table, cs.table_host, cs.first_row, cs.B = d.data_ptr(), h.data_ptr(), 0, 2
        cs.ind, cs.min_dist, cs.codes, cs.dist, cs.n_dst, cs.E = ind.data_ptr(), md.data_ptr(), codes.data_ptr(), dist.data_ptr(), 14, E
        return mt, cs, (d, h)

    for field, value, kind in (("avail", 29, L.OP_MEL_TILE), ("src", 23, L.OP_MEL_TILE), ("pitch", 27, L.OP_MEL_TILE),
                               ("n_valid", 8, L.OP_CODE_STITCH), ("dst", 8, L.OP_CODE_STITCH), ("dst", -1, L.OP_CODE_STITCH)):
        tbl = good.copy()
        tbl[field][1] = value
        mt, cs, keep = ops(tbl)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(kind, mt if kind == L.OP_MEL_TILE else cs)
    for field in ("table", "table_host", "mel", "in_mel"):
        mt, cs, keep = ops(good)
        setattr(mt, field, None)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(L.OP_MEL_TILE, mt)
    for field, value in (("ind", None), ("codes", None), ("B", 0), ("E", 6)):
        mt, cs, keep = ops(good)
        setattr(cs, field, value)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(L.OP_CODE_STITCH, cs)
    torch.cuda.synchronize()
    assert (in_mel == -7.0).all() and (codes == -9).all() and (dist == -9.0).all()


# ---- encode_utterances against encode() on hand-cut windows ---------------------------------------------------------
ENGINE_STATE = ("emb", "ema_numer", "ema_denom", "ind_hist", "zn_sum", "loss_buf", "met_buf", "diag")


def _engine_state(eng):
    return {n: getattr(eng, n).clone() for n in ENGINE_STATE if getattr(eng, n, None) is not None}


def _by_hand(m, mels, E, s, rf):
    """Per utterance (codes, dist) from model.encode() - the one-window call - on windows cut and zero-padded by hand."""
    out = []
    for mel in mels:
        wins, keep = UE.cut_windows(mel.cpu().numpy(), E, s, rf)
        cs, ds = [], []
        for w, k in enumerate(keep):
            c, d = m.encode(_dev(wins[w:w + 1]), return_dist=True)
            cs.append(c[0, :k])
            ds.append(d[0, :k])
        out.append((torch.cat(cs) if cs else torch.zeros(0, dtype=torch.int64, device=DEV),
                    torch.cat(ds) if ds else torch.zeros(0, device=DEV)))
    return out


@pytest.mark.parametrize("bn", ["vqvae", "vqvae-ema"])
def test_encode_utterances_equals_encode_on_hand_cut_windows(bn):
    hps, m, (wav, mel1, voice, jit) = _model(bn)
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    assert (E, mel_len) == (m.embed_len, m.enc_in_mel_len)
    frames = UE.mixed_frames(E, s, rf)
    gen = torch.Generator().manual_seed(5)
    mels = [torch.randn(39, F, generator=gen).to(DEV) for F in frames]
    ref = _by_hand(m, mels, E, s, rf)
    N = [UE.n_codes(F, s, rf) for F in frames]
    assert [c.numel() for c, _ in ref] == N and N[UE.MIX.index(0)] == 0
    voices = torch.arange(len(frames)) % 40
    eng = m._ensure_engine(B3)
    before = _engine_state(eng)
    assert "emb" in before and "loss_buf" in before and (bn != "vqvae-ema" or "ema_numer" in before)
    uc = m.encode_utterances(mels, voice=voices, batch=B3, return_dist=True, names=[f"u{i}" for i in range(len(frames))])
    assert m._engine is eng and eng.B == B3
    for n, t in _engine_state(eng).items():                                   # nothing of the codebook, the statistics,
        assert torch.equal(_bits(t), _bits(before[n])), n                     # the loss or the metric words moved
    assert isinstance(uc, CD.UtteranceCodes) and len(uc) == len(frames)
    assert uc.codes.dtype == torch.int64 and uc.codes.device.type == "cuda" and uc.dist.dtype == torch.float32
    assert uc.offsets.tolist() == np.concatenate([[0], np.cumsum(N)]).tolist()
    assert torch.equal(uc.voice, voices) and uc.names[3] == "u3"
    for u, (c, d) in enumerate(ref):                                          # bit for bit, for every code
        assert torch.equal(uc.row(u), c), u
        assert torch.equal(_bits(uc.dist[uc._off[u]:uc._off[u + 1]]), _bits(d)), u
    assert 0 <= int(uc.codes.min()) and int(uc.codes.max()) < hps.bn_vq_n_embed
    # the batch size and the order of the utterances do not change a bit
    for batch in (1, 16):
        other = m.encode_utterances(mels, batch=batch, return_dist=True)
        assert m._engine.B == batch
        assert torch.equal(other.codes, uc.codes) and torch.equal(_bits(other.dist), _bits(uc.dist)), batch
    rev = m.encode_utterances(mels[::-1], batch=B3, return_dist=True)
    for u in range(len(frames)):
        r = len(frames) - 1 - u
        assert torch.equal(rev.row(r), uc.row(u)), u
        # (random weights spread the frames over few codes; the distances tell every frame from every other)
        assert torch.equal(_bits(rev.dist[rev._off[r]:rev._off[r + 1]]), _bits(uc.dist[uc._off[u]:uc._off[u + 1]])), u
    # the default batch is the live engine's; units() are code_runs of a row; an empty call is an empty result
    assert m.encode_utterances(mels[:2])._off == [0, N[0], N[0] + N[1]] and m._engine.B == B3
    long = int(np.argmax(N))
    units, lengths, n_runs = uc.units(long)
    assert int(lengths.sum()) == N[long] and int(units[0]) == int(uc.row(long)[0]) and 1 <= int(n_runs) <= N[long]
    assert uc.padded().shape == (len(frames), max(N))
    none = m.encode_utterances([])
    assert len(none) == 0 and none.codes.numel() == 0
    with pytest.raises(L.AewError):
        m.encode_utterances([torch.zeros(38, 40, device=DEV)])
    # towards a pending backward it is what encode() is
    m.train()
    _, _, stale = m.run(wav, mel1, voice, jit)
    m.encode_utterances(mels[:3], batch=1)
    with pytest.raises(L.AewError, match="overwrote the activations"):
        stale.backward()


def test_whole_utterance_encoding_does_not_synchronise_the_host():
    hps, m, _ = _model("vqvae-ema")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    mf = DeviceMfcc(DEV, hps.sample_rate, hps.mfcc_win_sz, hps.mfcc_hop_sz, hps.n_mels, hps.n_mfcc)
    rs = np.random.RandomState(3)
    wavs = [_dev(_wav_for(mf, F, rs)) for F in (mel_len + s, rf, 2 * mel_len)]
    mels = [mf(w[None])[0] for w in wavs]
    warm = m.encode_utterances(mels, batch=B3, return_dist=True)     # builds the engine, its plans and graphs
    warm_w = m.encode_wavs(wavs, batch=B3, return_dist=True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                          # .item() / .cpu() / a blocking copy would raise
    try:
        got = m.encode_utterances(mels, batch=B3, return_dist=True, voice=[1, 2, 3])
        got_w = m.encode_wavs(wavs, batch=B3, return_dist=True)
        rows = [got.row(u) for u in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(got.codes, warm.codes) and torch.equal(got_w.codes, warm_w.codes)
    assert torch.equal(got.codes, got_w.codes)
    assert [r.numel() for r in rows] == [UE.n_codes(F, s, rf) for F in (mel_len + s, rf, 2 * mel_len)]


def test_encode_utterances_needs_discrete_codes():
    from ae_wavenet_amd import autoencoder_model as ae, config
    hps = config.make_hps("ae", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64, bn_n_out=16,
                          n_win_batch=96, n_blocks=2, n_block_layers=4)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    for call in (lambda: m.encode_utterances([torch.zeros(39, 40, device=DEV)]),
                 lambda: m.encode_wavs([torch.zeros(8000, device=DEV)])):
        with pytest.raises(L.AewError, match="discrete codes"):
            call()


# ---- against the oracle: the whole mel through the exact chain -------------------------------------------------------
def test_utterance_indices_equal_the_exact_oracle_over_the_whole_mel():
    from oracle import exact
    from tests.test_gpu_parity import seeded_full_engine
    hps, eng, wts, emb, inp = seeded_full_engine(B=2, w=100)
    E, s, rf, mel_len = G.utterance_geometry(eng.geom)
    F = rf + s * (3 * E + E // 2 - 1)                                         # three windows plus a partial one
    N = UE.n_codes(F, s, rf)
    assert N == 3 * E + E // 2 and 0 < E // 2 < E
    mel = np.random.RandomState(17).standard_normal((39, F)).astype(np.float32)
    plan = CD.tile_plan([F], E, s, rf, eng.B)
    assert plan.n_rows == 4 and plan.n_batches == 2
    codes = torch.full((N,), -1, dtype=torch.int64, device=DEV)
    dist = torch.full((N,), -1.0, device=DEV)
    eng.encode_tiles(_dev(mel).reshape(-1), plan.table([0]), codes, dist)
    torch.cuda.synchronize()
    ze = exact.linear_cl(exact.encoder_cl(wts, "encoder.", np.ascontiguousarray(mel.T)[None]), wts["bottleneck.linear.weight"])
    ind, d, _ = exact.vq_nearest(ze.reshape(-1, ze.shape[2]), emb, "scaled_l2")
    assert ze.shape[1] == N
    assert np.array_equal(codes.cpu().numpy(), ind)
    assert np.array_equal(dist.cpu().numpy(), d)


# ---- encode_wavs / encode_corpus ---------------------------------------------------------------------------------------
def _wav_for(mf, frames, rs, loud_from=None):
    """mu-law-like values for an utterance of `frames` mel frames: random over the whole range; with loud_from, the
    samples in front of it are a whisper: noise of amplitude 1e-3 around zero, with no offset whose spectral leakage
    would set the same floor in both halves - about 100 dB under the loud part, beyond the 80 dB the transform keeps."""
    n = next(n for n in range(frames * mf.hop, (frames + 4) * mf.hop) if mf.n_frames(n) == frames)
    w = rs.randint(0, 256, n).astype(np.float32)
    if loud_from is not None:
        w[:loud_from] = 1e-3 * rs.standard_normal(loud_from).astype(np.float32)
    return w


def test_encode_wavs_uses_the_whole_utterance_mfcc():
    hps, m, _ = _model("vqvae-ema")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    mf = DeviceMfcc(DEV, hps.sample_rate, hps.mfcc_win_sz, hps.mfcc_hop_sz, hps.n_mels, hps.n_mfcc)
    rs = np.random.RandomState(23)
    F = [rf + s * (2 * E + 2), rf - 1, mel_len, 3]                            # three windows; no code; one window; no frame
    wavs = [_dev(_wav_for(mf, f, rs)) for f in F]
    wavs[0] = _dev(_wav_for(mf, F[0], rs, loud_from=(mel_len + 8) * mf.hop))    # window 0 lies in the whisper
    got = m.encode_wavs(wavs, batch=B3, return_dist=True, voice=[4, 5, 6, 7])
    mels = [mf(w[None])[0] if f >= mf.MIN_FRAMES else torch.zeros(39, 0, device=DEV) for w, f in zip(wavs, F)]
    assert [x.shape[1] for x in mels] == [F[0], F[1], F[2], 0]
    want = m.encode_utterances(mels, batch=B3, return_dist=True)
    assert got._off == want._off == [0, 2 * E + 3, 2 * E + 3, 3 * E + 3, 3 * E + 3]
    assert torch.equal(got.codes, want.codes) and torch.equal(_bits(got.dist), _bits(want.dist))
    assert got.voice.tolist() == [4, 5, 6, 7]
    # the ragged front-end IS the whole-utterance MFCC, and holds one scratch buffer whatever the lengths
    flat, frames, bases = m._utt_mfcc.ragged(wavs)
    assert frames == [F[0], F[1], F[2], 0] and torch.equal(_bits(flat[:39 * F[0]].view(39, F[0])), _bits(mels[0]))
    scratch = m._utt_mfcc._ragged_scratch
    m._utt_mfcc.ragged(wavs[2:])
    assert m._utt_mfcc._ragged_scratch is scratch and not m._utt_mfcc._plans
    # per-window MFCC tiling gives something else where the utterance's loud part sets the floor: window 0, computed on
    # its own samples alone, keeps the whisper's spectrum; in the whole-utterance transform it lies under the dB floor
    alone = mf(wavs[0][None, :m.enc_in_len])[0]
    assert alone.shape == (39, mel_len)
    inner = slice(4, mel_len - 4)                                              # (away from the delta filters' edge rows)
    assert not torch.equal(alone[:13, inner], mels[0][:13, inner])
    c_alone, d_alone = m.encode(alone[None], return_dist=True)
    assert not torch.equal(_bits(d_alone[0]), _bits(got.dist[:E]))


def test_encode_corpus_equals_per_utterance_encode_wavs():
    hps, m, _ = _model("vqvae")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    mf = DeviceMfcc(DEV, hps.sample_rate, hps.mfcc_win_sz, hps.mfcc_hop_sz, hps.n_mels, hps.n_mfcc)
    rs = np.random.RandomState(31)
    F = [mel_len + s, rf, 2 * mel_len, rf + 5, mel_len - 1]
    parts = [_wav_for(mf, f, rs).astype(np.uint8) for f in F]
    gap = 7                                                                    # the utterances do not touch in snd_data
    snd, samples, at = [], [], 3
    snd.append(np.zeros(at, np.uint8))
    for i, p in enumerate(parts):
        samples.append(CP.SpokenSample(voice_index=(7 * i) % 5, wav_b=at, wav_e=at + len(p), file_path=f"spk{i}/utt{i}.flac"))
        snd += [p, np.zeros(gap, np.uint8)]
        at += len(p) + gap
    corpus = CP.DeviceCorpus.from_arrays(np.concatenate(snd), samples, 1000, 500, DEV)
    got = m.encode_corpus(corpus, batch=B3, return_dist=True)
    N = [UE.n_codes(f, s, rf) for f in F]
    assert len(got) == 5 and got._off == np.concatenate([[0], np.cumsum(N)]).tolist()
    assert got.voice.tolist() == [0, 2, 4, 1, 3] and got.names == [f"spk{i}/utt{i}.flac" for i in range(5)]
    for u, p in enumerate(parts):
        one = m.encode_wavs([_dev(p.astype(np.float32))], batch=B3, return_dist=True)
        assert torch.equal(one.codes, got.row(u)), u
        assert torch.equal(_bits(one.dist), _bits(got.dist[got._off[u]:got._off[u + 1]])), u
    for chunk in (1, F[0] + F[1], 10 ** 9):                                    # one utterance, two, all per chunk
        other = m.encode_corpus(corpus, batch=B3, max_frames_per_chunk=chunk, return_dist=True)
        assert torch.equal(other.codes, got.codes) and torch.equal(_bits(other.dist), _bits(got.dist)), chunk
        assert other._off == got._off and other.names == got.names
    with pytest.raises(L.AewError):
        m.encode_corpus(CP.DeviceCorpus.from_arrays(np.concatenate(snd), samples, 1000, 500, None))


# ---- one batch from a captured graph ------------------------------------------------------------------------------------
def test_a_captured_batch_follows_new_input():
    hps, m, _ = _model("vqvae-ema")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    eng = m._ensure_engine(B3)
    frames = [rf + s * (E + 2), mel_len]                                       # two windows + one: one batch of three rows
    plan = CD.tile_plan(frames, E, s, rf, B3)
    assert plan.n_batches == 1 and plan.n_rows == 3
    bases, n_src = UE.bases_of(frames, 39)
    tbl = plan.table(bases)
    host = _pinned(tbl)
    dev = host.to(DEV)
    mel = torch.zeros(n_src, device=DEV)
    codes = torch.full((plan.n_codes + CANARY,), -9, dtype=torch.int64, device=DEV)
    dist = torch.full((plan.n_codes + CANARY,), -9.0, device=DEV)
    p = eng.utterance_batch_plan(mel, dev, host, 0, codes[:plan.n_codes], dist[:plan.n_codes])
    assert p.labels[0] == "utt.tile" and p.labels[-1] == "utt.stitch" and "vq.stats" not in p.labels and len(p.ops) > 3
    gen = torch.Generator().manual_seed(9)
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(3):                                                      # capture + first launch, then two replays
        mels = [torch.randn(39, F, generator=gen).to(DEV) for F in frames]
        mel.copy_(torch.cat([x.reshape(-1) for x in mels]))
        codes.fill_(-9)
        p.run_graph(st)
        assert p._graph is not None
        want = m.encode_utterances(mels, batch=B3, return_dist=True)
        assert torch.equal(codes[:plan.n_codes], want.codes) and torch.equal(_bits(dist[:plan.n_codes]), _bits(want.dist)), rep
        assert (codes[plan.n_codes:] == -9).all() and (dist[plan.n_codes:] == -9.0).all()
    # the table is read on the device at every replay: with the second utterance's row made idle its codes stay away
    idle = tbl.copy()
    idle[2] = (0, 0, 0, 0, 0, 0)
    dev.copy_(_dev(idle.view(np.uint8).reshape(-1)))
    codes.fill_(-9)
    p.run_graph(st)
    n0 = int(plan.offsets[1])
    assert torch.equal(codes[:n0], want.codes[:n0]) and (codes[n0:] == -9).all()
    p.invalidate_graph()
