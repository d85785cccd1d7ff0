"""Penalised Viterbi decoding of codes on the device: AEW_OP_CODE_SEGMENT bit for bit against the numpy restatement
(tests/segment_emulator.py) on the shape list the host twin passes on the CPU - the slab and group edges of k_seg_cost
and the ballot-word edges of k_seg_scan are named there -, AEW_OP_FRAME_STITCH against the rows it moves, records
tampered with on the device, one captured launch replayed on new frames, and model.segment_utterances() /
segment_wavs() / segment_corpus() against the encode_* calls they extend."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, codes as CD, corpus as CP, geometry as G
from ae_wavenet_amd.mfcc import DeviceMfcc
from ae_wavenet_amd.plan import Plan
from tests import segment_emulator as SE, utterance_emulator as UE
from tests.test_codes_gpu import _bits, _model
from tests.test_segment_cpu import CASES, check_against_emulator
from tests.test_utterance_gpu import ENGINE_STATE, _engine_state, _wav_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 8
B3 = 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pinned(tbl):
    host = torch.empty(max(tbl.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    host.numpy()[:tbl.nbytes] = tbl.view(np.uint8).reshape(-1)
    return host


class _Launch:
    """One AEW_OP_CODE_SEGMENT over a case, outputs with canaries behind them; everything it points to is kept."""

    def __init__(self, case, dist=True):
        self.case = case
        frames, emb, off = case["frames"], case["emb"], case["offsets"]
        n, d_pitch = frames.shape
        K = len(emb)
        self.n, self.U = n, len(off) - 1
        self.plan = CD.segment_plan(np.diff(off), K)
        self.tbl = self.plan.table
        self.tbl["lam"] = case["lams"]
        self.host = _pinned(self.tbl)
        self.table = self.host.to(DEV)
        self.frames, self.emb = _dev(frames), _dev(emb)
        self.codes = torch.full((n + CANARY,), -9, dtype=torch.int64, device=DEV)
        self.dist = torch.full((n + CANARY,), -9.0, dtype=torch.float32, device=DEV)
        self.cost = torch.full((self.U + CANARY,), -9.0, dtype=torch.float32, device=DEV)
        self.n_seg = torch.full((self.U + CANARY,), -9, dtype=torch.int32, device=DEV)
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(max(self.plan.ws_bytes // 8, 1), dtype=torch.int64, device=DEV)
        cs = L.CodeSegment()
        cs.frames, cs.n_elems = self.frames.data_ptr(), self.frames.numel()
        cs.emb, cs.K, cs.d, cs.d_pitch, cs.metric = self.emb.data_ptr(), K, case["d"], d_pitch, CD.VQ_METRICS[case["metric"]]
        cs.table, cs.table_host, cs.U = self.table.data_ptr(), self.host.data_ptr(), self.U
        cs.codes, cs.dist, cs.n_out = self.codes.data_ptr(), (self.dist.data_ptr() if dist else None), n
        cs.cost, cs.n_seg, cs.n_bad = self.cost.data_ptr(), self.n_seg.data_ptr(), self.n_bad.data_ptr()
        cs.ws, cs.ws_bytes = self.ws.data_ptr(), self.plan.ws_bytes
        self.rec = cs

    def run(self):
        CD._run(L.OP_CODE_SEGMENT, self.rec, "segment op", torch.device(DEV))
        return self.read()

    def read(self):
        n, U = self.n, self.U
        codes, dist, cost, n_seg = (t.cpu().numpy() for t in (self.codes, self.dist, self.cost, self.n_seg))
        assert (codes[n:] == -9).all() and (dist[n:] == -9.0).all() and (cost[U:] == -9.0).all() and (n_seg[U:] == -9).all()
        return codes[:n], dist[:n], cost[:U], n_seg[:U], int(self.n_bad.cpu()[0]) & 0xFFFFFFFF


# ---- the op alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernels_equal_the_emulator_bit_for_bit(case):
    """K in {1, 3, 64, 65, 130, 256, 257, 4096}; T in {1, 2, 0, 63, 64, 65, 129} mixed in one launch, each utterance with
    its own penalty (0, mid values, 1e30, inf); d in {1, 3, 32, 64, 65} with d_pitch > d and NaN in the pad channels; both
    metrics; duplicated rows and equal r at a switch; a NaN frame in the middle of an utterance (n_bad = 1).  324 rows =
    five slabs of 64 frames and four rows, 108 = one slab and 44; K = 256 one whole group of entries, 257 one more."""
    check_against_emulator(case, _Launch(case).run())


def test_without_dist_and_the_functional_form():
    case = next(c for c in CASES if c["name"] == "K130-scaled_l2")
    la = _Launch(case, dist=False)
    codes, dist, cost, n_seg, n_bad = la.run()
    want = SE.expected(case)
    assert np.array_equal(codes, want[0]) and (dist == -9.0).all() and np.array_equal(n_seg, want[3])
    c2, d2, cost2, seg2 = CD.segment(la.frames, case["offsets"], la.emb[:, :case["d"]], case["lams"], case["metric"], return_dist=True)
    assert np.array_equal(c2.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(cost2.cpu().numpy().view(np.uint32), want[2].view(np.uint32)) and np.array_equal(seg2.cpu().numpy(), want[3])
    c3, cost3, seg3 = CD.segment(la.frames, case["offsets"], la.emb, 0.0, case["metric"])
    near = SE.segment_ragged(case["frames"][:, :case["d"]].copy(), case["offsets"], case["emb"], case["metric"],
                             np.zeros(len(case["lams"]), np.float32))
    assert np.array_equal(c3.cpu().numpy(), near[0]) and np.array_equal(seg3.cpu().numpy(), near[3])
    with pytest.raises(L.AewError, match="penalty"):
        CD.segment(la.frames, case["offsets"], la.emb, -1.0)
    with pytest.raises(L.AewError, match="GPU only"):
        CD.segment(la.frames.cpu(), case["offsets"], la.emb.cpu(), 1.0)


def test_the_functional_form_does_not_synchronise_the_host():
    case = next(c for c in CASES if c["name"] == "K65-sq_l2")
    frames, emb = _dev(case["frames"]), _dev(case["emb"])
    warm = CD.segment(frames, case["offsets"], emb, case["lams"], "sq_l2", return_dist=True)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = CD.segment(frames, case["offsets"], emb, case["lams"], "sq_l2", return_dist=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
               for a, b in zip(got, warm))


def test_a_record_tampered_with_on_the_device_leaves_its_outputs_alone():
    """The launcher checks the host copy; the kernels repeat the check on the device copy and leave alone what fails it."""
    case = SE.make_case("tamper", 70, 4, 4, (6, 9, 5), "sq_l2", 13)
    want = SE.expected(case)
    for field, value in (("first_frame", 12), ("first_frame", -1), ("n_frames", 15), ("back_base", 12 * 3), ("lam", -1.0),
                         ("n_frames", -2)):
        la = _Launch(case)
        bad = la.tbl.copy()
        bad[field][1] = value
        la.table.copy_(_dev(bad.view(np.uint8).reshape(-1)))
        codes, dist, cost, n_seg, n_bad = la.run()
        for u, (lo, hi) in enumerate(((0, 6), (6, 15), (15, 20))):
            if u == 1:
                assert (codes[lo:hi] == -9).all() and (dist[lo:hi] == -9.0).all() and cost[u] == -9.0 and n_seg[u] == -9, (field, value)
            else:
                assert np.array_equal(codes[lo:hi], want[0][lo:hi]) and cost[u] == want[2][u] and n_seg[u] == want[3][u], (field, value)
    # refused on the host: nothing is launched
    la = _Launch(case)
    la.host.numpy().view(L.SEG_UTT_DTYPE)["lam"][2] = np.nan
    with pytest.raises(L.AewError, match="rc=-1"):
        la.run()
    la = _Launch(case)
    la.rec.ws_bytes -= 8
    with pytest.raises(L.AewError, match="rc=-1"):
        la.run()
    torch.cuda.synchronize()
    assert (la.codes == -9).all() and (la.cost == -9.0).all()


def test_a_captured_launch_follows_new_frames():
    case = SE.make_case("graph", 130, 8, 12, (33, 0, 70), "scaled_l2", 14)
    la = _Launch(case)
    p = Plan("segment")
    p.add(L.OP_CODE_SEGMENT, la.rec, "code.segment")
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(3):                                                      # capture + first launch, then two replays
        other = SE.make_case(f"graph{rep}", 130, 8, 12, (33, 0, 70), "scaled_l2", 14 + rep)
        la.frames.copy_(_dev(other["frames"]))
        other["emb"] = case["emb"]
        la.codes.fill_(-9)
        la.n_bad.zero_()
        p.run_graph(st)
        assert p._graph is not None
        check_against_emulator(other, la.read())
    p.invalidate_graph()


# ---- AEW_OP_FRAME_STITCH ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_pitch,shift", [(64, 0), (8, 0), (6, 0), (64, 1)])
def test_frame_stitch_moves_the_rows_the_windows_own(d_pitch, shift):
    """An utterance of three windows (and two short ones, and the idle rows of the last batch): the stitched frames are the
    bits of `lin` of the windows that own them.  (64, 0) and (8, 0): 16-byte moves; (6, 0): a pitch that allows none;
    (64, 1): a destination off 16 bytes - the element path."""
    E = 7
    s, rf = G.encoder_stride_rf()
    frames = [rf + s * (2 * E + 2), rf, rf + s * (E - 1), 3]                    # 3 windows, 1 code, a full window, no code
    plan = CD.tile_plan(frames, E, s, rf, B3)
    assert plan.n_rows == 5 and plan.n_batches == 2 and (plan.utt[:3] == 0).all()
    tbl = plan.table(UE.bases_of(frames, 5)[0])
    host, n_dst = _pinned(tbl), plan.n_codes
    table = host.to(DEV)
    out = torch.full((shift + (n_dst + 2) * d_pitch,), -7.0, dtype=torch.float32, device=DEV)
    want = np.full((n_dst + 2) * d_pitch, -7.0, np.float32)
    rs = np.random.RandomState(d_pitch)
    lin_bs = (E + 1) * d_pitch                                                 # a batch stride with a row to spare
    for first in range(0, len(tbl), B3):
        lin = rs.standard_normal(B3 * lin_bs).astype(np.float32)
        lin[::5] = np.float32(-0.0)                                            # bytes, not values
        lin_d = _dev(lin)
        fs = L.FrameStitch()
        fs.table, fs.table_host, fs.first_row, fs.B = table.data_ptr(), host.data_ptr(), first, B3
        fs.lin, fs.lin_bs, fs.frames, fs.n_dst = lin_d.data_ptr(), lin_bs, out.data_ptr() + 4 * shift, n_dst
        fs.E, fs.d_pitch = E, d_pitch
        CD._run(L.OP_FRAME_STITCH, fs, "frame stitch", torch.device(DEV))
        for b in range(B3):
            r = tbl[first + b]
            nv, dst = int(r["n_valid"]), int(r["dst"])
            want[dst * d_pitch:(dst + nv) * d_pitch] = lin[b * lin_bs:b * lin_bs + nv * d_pitch]
        got = out.cpu().numpy()
        assert (got[:shift] == -7.0).all() and got[shift:].tobytes() == want.tobytes(), first
    assert not (want[:n_dst * d_pitch] == -7.0).any() and (want[n_dst * d_pitch:] == -7.0).all()
    # a record tampered with on the device stores nothing; one that is wrong on the host is refused before the launch
    out.fill_(-7.0)
    bad = tbl.copy()
    bad["dst"][0], bad["n_valid"][1], bad["dst"][2] = n_dst - 1, E + 1, -1
    table.copy_(_dev(bad.view(np.uint8).reshape(-1)))
    fs.first_row = 0
    CD._run(L.OP_FRAME_STITCH, fs, "frame stitch", torch.device(DEV))
    assert (out == -7.0).all()
    host.numpy()[:] = bad.view(np.uint8).reshape(-1)
    with pytest.raises(L.AewError, match="rc=-1"):
        CD._run(L.OP_FRAME_STITCH, fs, "frame stitch", torch.device(DEV))
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---- the surface ---------------------------------------------------------------------------------------------------------
def _runs(row):
    r = row.cpu().numpy()
    return 0 if not len(r) else 1 + int((r[1:] != r[:-1]).sum())


@pytest.mark.parametrize("bn", ["vqvae", "vqvae-ema"])
def test_segment_utterances_extends_encode_utterances(bn):
    hps, m, _ = _model(bn)
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    frames = UE.mixed_frames(E, s, rf)
    gen = torch.Generator().manual_seed(5)
    mels = [torch.randn(39, F, generator=gen).to(DEV) for F in frames]
    U = len(frames)
    voices = torch.arange(U) % 40
    plain = m.encode_utterances(mels, batch=B3, return_dist=True)
    eng = m._engine
    before = _engine_state(eng)
    assert "emb" in before and "loss_buf" in before and (bn != "vqvae-ema" or "ema_numer" in before)
    # penalty 0: the nearest codes and their distances, bit for bit
    got, info = m.segment_utterances(mels, 0, voice=voices, batch=B3, return_dist=True, names=[f"u{i}" for i in range(U)],
                                     return_info=True)
    assert isinstance(got, CD.UtteranceCodes) and isinstance(info, CD.Segmentation) and m._engine is eng
    assert got._off == plain._off and torch.equal(got.codes, plain.codes) and torch.equal(_bits(got.dist), _bits(plain.dist))
    assert torch.equal(got.voice, voices) and got.names[3] == "u3" and int(info.n_bad[0]) == 0
    runs = [_runs(plain.row(u)) for u in range(U)]
    assert info.n_segments.tolist() == runs
    # a positive penalty: no more segments than the plain codes have runs; the cost is the objective of the labelling
    lam = float(plain.dist.median()) * 0.02
    seg, sinfo = m.segment_utterances(mels, lam, batch=B3, return_dist=True, return_info=True)
    nseg = sinfo.n_segments.tolist()
    print(f"{bn}: runs of the plain codes {runs}, segments at penalty {lam:.4g} {nseg}")
    assert seg._off == plain._off and all(a <= b for a, b in zip(nseg, runs))
    assert nseg == [_runs(seg.row(u)) for u in range(U)]
    assert sinfo.penalty.tolist() == [np.float32(lam)] * U
    for u in range(U):
        n = seg._off[u + 1] - seg._off[u]
        want = float(seg.dist[seg._off[u]:seg._off[u + 1]].double().sum()) + float(np.float32(lam)) * max(nseg[u] - 1, 0)
        assert abs(float(sinfo.cost[u]) - want) <= 4 * (n + 16) * 2.0 ** -24 * max(want, 1e-30), u
    one = m.segment_utterances(mels, float("inf"), batch=B3)
    assert all(_runs(one.row(u)) <= 1 for u in range(U))
    # nothing of the codebook, the statistics, the loss or the metric words moved
    assert m._engine is eng
    for n, t in _engine_state(eng).items():
        assert torch.equal(_bits(t), _bits(before[n])), n
    # a penalty per utterance, and the batch size, change nothing else
    lams = [0.0 if u % 2 else lam for u in range(U)]
    mixed = m.segment_utterances(mels, lams, batch=1, return_dist=True)
    for u in range(U):
        src = plain if u % 2 else seg
        assert torch.equal(mixed.row(u), src.row(u)), u
    assert m._engine.B == 1
    m.segment_utterances(mels, lam, batch=B3)
    assert m._engine.B == B3
    # the codes are codes: units, edit distance
    from ae_wavenet_amd import align
    long = int(np.argmax(nseg))
    units, lengths, n_runs = seg.units(long)
    assert int(n_runs) == nseg[long] and int(lengths.sum()) == seg.row(long).numel()
    ed = align.edit_distance(seg, plain, collapse=True)
    assert ed.distance.numel() == U
    none = m.segment_utterances([], 1.0)
    assert len(none) == 0 and none.codes.numel() == 0
    for pen in (-1.0, float("nan"), [1.0, 2.0]):
        with pytest.raises(L.AewError, match="penalty"):
            m.segment_utterances(mels, pen)


def test_segment_utterances_needs_discrete_codes():
    from ae_wavenet_amd import autoencoder_model as ae, config
    hps = config.make_hps("ae", n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64, bn_n_out=16,
                          n_win_batch=96, n_blocks=2, n_block_layers=4)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    for call in (lambda: m.segment_utterances([torch.zeros(39, 40, device=DEV)], 1.0),
                 lambda: m.segment_wavs([torch.zeros(8000, device=DEV)], 1.0)):
        with pytest.raises(L.AewError, match="discrete codes"):
            call()


def test_segment_wavs_and_segment_corpus():
    hps, m, _ = _model("vqvae-ema")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    mf = DeviceMfcc(DEV, hps.sample_rate, hps.mfcc_win_sz, hps.mfcc_hop_sz, hps.n_mels, hps.n_mfcc)
    rs = np.random.RandomState(31)
    F = [mel_len + s, rf, 2 * mel_len, rf + 5, mel_len - 1]
    parts = [_wav_for(mf, f, rs).astype(np.uint8) for f in F]
    wavs = [_dev(p.astype(np.float32)) for p in parts]
    plain = m.encode_wavs(wavs, batch=B3, return_dist=True)
    zero = m.segment_wavs(wavs, 0.0, batch=B3, return_dist=True, voice=[4, 5, 6, 7, 8])
    assert zero._off == plain._off and torch.equal(zero.codes, plain.codes) and torch.equal(_bits(zero.dist), _bits(plain.dist))
    assert zero.voice.tolist() == [4, 5, 6, 7, 8]
    snd, samples, at = [np.zeros(3, np.uint8)], [], 3
    for i, p in enumerate(parts):
        samples.append(CP.SpokenSample(voice_index=(7 * i) % 5, wav_b=at, wav_e=at + len(p), file_path=f"spk{i}/utt{i}.flac"))
        snd += [p, np.zeros(7, np.uint8)]
        at += len(p) + 7
    corpus = CP.DeviceCorpus.from_arrays(np.concatenate(snd), samples, 1000, 500, DEV)
    lam = [float(plain.dist.median()) * f for f in (0.5, 0.0, 1.0, 0.25, 2.0)]
    want, winfo = m.segment_wavs(wavs, lam, batch=B3, return_dist=True, return_info=True)
    got, info = m.segment_corpus(corpus, lam, batch=B3, return_dist=True, return_info=True)
    assert got.voice.tolist() == [0, 2, 4, 1, 3] and got.names == [f"spk{i}/utt{i}.flac" for i in range(5)]
    for chunk in (1, F[0] + F[1]):                                             # one utterance, two per chunk
        other, oinfo = m.segment_corpus(corpus, lam, batch=B3, max_frames_per_chunk=chunk, return_dist=True, return_info=True)
        for a, b in ((other, got), (want, got)):
            assert a._off == b._off and torch.equal(a.codes, b.codes) and torch.equal(_bits(a.dist), _bits(b.dist)), chunk
        for a, b in ((oinfo, info), (winfo, info)):
            assert torch.equal(_bits(a.cost), _bits(b.cost)) and torch.equal(a.n_segments, b.n_segments)
            assert torch.equal(_bits(a.penalty), _bits(b.penalty)) and int(a.n_bad[0]) == int(b.n_bad[0]) == 0
    assert torch.equal(got.row(1), plain.row(1))                               # (penalty 0 for that one)


def test_decode_utterances_accepts_a_segmentation():
    from tests.test_cond_utterance_gpu import _model as _model_1000
    hps, m, _ = _model_1000("vqvae-ema")
    E, s, rf, mel_len = G.utterance_geometry(m.geom)
    mel = torch.randn(39, rf + s * 8, generator=torch.Generator().manual_seed(3)).to(DEV)      # 9 codes: 708 samples
    plain = m.encode_utterances([mel], batch=B3, return_dist=True)
    seg = m.segment_utterances([mel], float(plain.dist.median()), voice=[7], batch=B3)
    assert seg.row(0).numel() == 9
    out = m.decode_utterances(seg, seed=5, batch=B3)
    assert len(out) == 1 and out[0].numel() == 708
