"""VQ codes as an interface, on the device: the lookup and run-length ops bit for bit against their numpy restatements
(tests/codes_emulator.py) with canaries behind every output, the run-length op from a captured graph, and the seam
between encoder and decoder - model.encode() / TrainEngine.codes_to_conditioning() / model.decode() / model.convert()
against conditioning() and sample(), which they must reproduce exactly."""
import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, autoencoder_model as ae, codes as CD, config, optim
from ae_wavenet_amd.plan import Plan
from tests import codes_emulator as CE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
RUN_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2500)     # (the kernel's chunk is 1024 positions)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- lookup ---------------------------------------------------------------------------------------------------------
def _lookup(emb, ind, d_pitch, with_bad=True, emb_shift=0):
    """One launch of the op on raw buffers: (zq [Q][d_pitch], bad count or None); the canary behind zq is checked here.
    emb_shift: the codebook starts that many floats into its buffer (4-byte aligned only: the scalar path)."""
    K, d = emb.shape
    Q = ind.size
    e_buf = torch.zeros(K * d + emb_shift, dtype=torch.float32, device=DEV)
    e_buf[emb_shift:].copy_(_dev(emb).reshape(-1))
    zq = torch.full((Q * d_pitch + CANARY,), -7.0, dtype=torch.float32, device=DEV)
    bad = torch.zeros(4, dtype=torch.int32, device=DEV)
    i_t = _dev(ind)
    lk = L.CodeLookup()
    lk.ind, lk.emb, lk.zq = i_t.data_ptr(), e_buf.data_ptr() + 4 * emb_shift, zq.data_ptr()
    lk.bad = bad.data_ptr() if with_bad else None
    lk.Q, lk.K, lk.d, lk.d_pitch = Q, K, d, d_pitch
    CD._run(L.OP_CODE_LOOKUP, lk, "code lookup", torch.device(DEV))
    out = zq.cpu().numpy()
    assert (out[Q * d_pitch:] == -7.0).all(), "canary behind zq"
    b = bad.cpu().numpy()
    assert not b[1:].any()
    return out[:Q * d_pitch].reshape(Q, d_pitch), (int(b[0]) if with_bad else None)


@pytest.mark.parametrize("K,d,d_pitch,Q,shift", [(128, 16, 16, 1, 0), (128, 10, 16, 5, 0), (4096, 64, 64, 257, 0),
                                                 (128, 16, 16, 5, 1)])
def test_lookup_equals_the_row_gather_bit_for_bit(K, d, d_pitch, Q, shift):
    rs = np.random.RandomState(K + Q)
    emb = rs.randn(K, d).astype(np.float32)
    emb[0, 0], emb[K - 1, d - 1] = np.float32(-0.0), np.float32("nan")          # bytes, not values
    ind = rs.randint(0, K, Q).astype(np.int64)
    ind[0], ind[-1] = K - 1, (0 if Q > 1 else K - 1)
    want, _ = CE.lookup(emb, ind, d_pitch)
    assert want[:, :d].tobytes() == emb[ind].tobytes()
    got, bad = _lookup(emb, ind, d_pitch, emb_shift=shift)
    assert got.tobytes() == want.tobytes() and bad == 0
    assert not got[:, d:].view(np.uint32).any()                                   # pad channels: zero bits
    if Q >= 5:                                                                    # indices outside the codebook
        pos = [0, Q // 2, Q - 1]
        bad_ind = ind.copy()
        bad_ind[pos] = [-1, K, np.iinfo(np.int64).max]
        want2, nbad = CE.lookup(emb, bad_ind, d_pitch)
        got2, bad2 = _lookup(emb, bad_ind, d_pitch, emb_shift=shift)
        assert nbad == 3 and bad2 == 3 and got2.tobytes() == want2.tobytes()
        keep = np.setdiff1d(np.arange(Q), pos)
        assert not got2[pos].view(np.uint32).any() and got2[keep].tobytes() == got[keep].tobytes()
        got3, none = _lookup(emb, bad_ind, d_pitch, with_bad=False, emb_shift=shift)
        assert none is None and got3.tobytes() == got2.tobytes()
    # the functional form: any shape of codes
    z = CD.lookup(_dev(emb), _dev(ind).view(1, Q), d_pitch=d_pitch)
    assert z.shape == (1, Q, d_pitch) and z.cpu().numpy().tobytes() == want.tobytes()


def test_lookup_refuses_malformed_records():
    emb, ind = torch.zeros(4, 4, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    zq = torch.zeros(3, 4, device=DEV)
    for field, v in (("Q", 0), ("K", 0), ("d", 0), ("d_pitch", 3), ("zq", None), ("ind", None)):
        lk = L.CodeLookup()
        lk.ind, lk.emb, lk.zq, lk.Q, lk.K, lk.d, lk.d_pitch = ind.data_ptr(), emb.data_ptr(), zq.data_ptr(), 3, 4, 4, 4
        setattr(lk, field, v)
        with pytest.raises(L.AewError, match="rc=-1"):
            CD._run(L.OP_CODE_LOOKUP, lk, "code lookup", torch.device(DEV))
    torch.cuda.synchronize()
    assert not zq.any()


# ---- runs -----------------------------------------------------------------------------------------------------------
def _runs_buffers(B, N, pitch):
    return dict(ind=torch.zeros(B * pitch + CANARY, dtype=torch.int64, device=DEV),
                units=torch.full((B * N + CANARY,), 99, dtype=torch.int64, device=DEV),
                lengths=torch.full((B * N + CANARY,), 99, dtype=torch.int32, device=DEV),
                n_runs=torch.full((B + CANARY,), 99, dtype=torch.int32, device=DEV))


def _runs_op(buf, B, N, pitch):
    cr = L.CodeRuns()
    cr.ind, cr.ind_pitch, cr.B, cr.N = buf["ind"].data_ptr(), pitch, B, N
    cr.units, cr.lengths, cr.n_runs = buf["units"].data_ptr(), buf["lengths"].data_ptr(), buf["n_runs"].data_ptr()
    return cr


def _set_rows(buf, rows, pitch):
    B, N = rows.shape
    padded = np.full((B, pitch), -5, np.int64)                       # what lies between the rows must not matter
    padded[:, :N] = rows
    buf["ind"][:B * pitch].copy_(_dev(padded).reshape(-1))


def _check_runs(buf, rows):
    B, N = rows.shape
    want = CE.code_runs(rows)
    for name, w, n in zip(("units", "lengths", "n_runs"), want, (B * N, B * N, B)):
        got = buf[name].cpu().numpy()
        assert got[:n].tobytes() == w.tobytes(), name
        assert (got[n:] == 99).all(), f"canary behind {name}"


@pytest.mark.parametrize("N", RUN_LENGTHS)
def test_runs_equal_the_emulator_bit_for_bit(N):
    rows = CE.boundary_rows(N)          # straddling runs, runs that start on the seams, all equal, all distinct, random
    for pick in ([0, 1, 2], [3, 4, 0]):                             # B = 3 rows of different content, pitch > N
        B, pitch = 3, N + 5
        buf = _runs_buffers(B, N, pitch)
        _set_rows(buf, rows[pick], pitch)
        CD._run(L.OP_CODE_RUNS, _runs_op(buf, B, N, pitch), "code runs", torch.device(DEV))
        _check_runs(buf, rows[pick])
    # the functional form, on a strided view (every second column of a wider tensor) and on one row
    wide = _dev(np.repeat(rows, 2, axis=1))
    u, ln, n = CD.code_runs(wide[:, ::2])
    want = CE.code_runs(rows)
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((u, ln, n), want))
    pitched = torch.full((rows.shape[0], N + 7), -5, dtype=torch.int64, device=DEV)      # rows used in place, by their pitch
    pitched[:, :N] = _dev(rows)
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(CD.code_runs(pitched[:, :N]), want))
    u1, l1, n1 = CD.code_runs(_dev(rows[4]))
    assert u1.shape == (N,) and int(n1) == want[2][4] and u1.cpu().numpy().tobytes() == want[0][4].tobytes()


def test_runs_over_an_utterance_length_row():
    """One row of 100 000 codes (98 chunks of the one workgroup that walks it), through the functional form."""
    N = 100000
    rs = np.random.RandomState(7)
    row = np.repeat(rs.randint(0, 512, N), rs.randint(1, 6, N))[:N].astype(np.int64)
    want = CE.code_runs(row[None])
    got = CD.code_runs(_dev(row))
    assert all(g.cpu().numpy().tobytes() == w[0].tobytes() for g, w in zip(got, want))
    assert 0 < int(got[2]) < N and int(got[1].sum()) == N


def test_runs_from_a_captured_graph_track_the_input():
    N, B, pitch = 1025, 3, 1100
    buf = _runs_buffers(B, N, pitch)
    plan = Plan("code_runs")
    plan.add(L.OP_CODE_RUNS, _runs_op(buf, B, N, pitch), "code.runs")
    rows = CE.boundary_rows(N)
    st = torch.cuda.current_stream().cuda_stream
    for pick in ([0, 1, 2], [3, 4, 0], [2, 2, 3]):                   # capture + first launch, then two replays
        _set_rows(buf, rows[pick], pitch)
        plan.run_graph(st)
        assert plan._graph is not None
        _check_runs(buf, rows[pick])
    plan.invalidate_graph()


def test_runs_refuse_empty_input():
    buf = _runs_buffers(2, 4, 4)
    for B, N, pitch in ((0, 4, 4), (2, 0, 4), (2, 4, 3)):
        with pytest.raises(L.AewError, match="rc=-1"):
            CD._run(L.OP_CODE_RUNS, _runs_op(buf, B, N, pitch), "code runs", torch.device(DEV))
    with pytest.raises(L.AewError):
        CD.code_runs(torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    assert (buf["units"] == 99).all() and (buf["n_runs"] == 99).all()


# ---- the seam: encode / codes_to_conditioning / decode against conditioning() and sample() ---------------------------
def _model(bn):
    """The small autoencoder of tests/test_sampler.py::test_autoencoder_eval_forward_samples_without_touching_the_codebook."""
    hps = config.make_hps(bn, n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64,
                          bn_n_out=16, bn_vq_n_embed=128, n_win_batch=96, n_blocks=2, n_block_layers=4)
    torch.manual_seed(0)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    g = m.geom
    gen = torch.Generator().manual_seed(1)
    args = (torch.randint(0, 256, (1, g.enc_in_len), generator=gen).float().to(DEV),
            torch.randn(1, 39, g.mel_len, generator=gen).to(DEV), torch.randint(0, 40, (1,), generator=gen).to(DEV),
            torch.arange(g.embed_len).repeat(1, 1).to(DEV))
    return hps, m, args


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _state(eng):
    return {n: getattr(eng, n).clone() for n in ("emb", "ema_numer", "ema_denom", "ind_hist") if hasattr(eng, n)}


@pytest.mark.parametrize("bn", ["vqvae", "vqvae-ema"])
def test_decode_from_encoded_codes_reproduces_conditioning_and_sample(bn):
    hps, m, (wav, mel, voice, jit) = _model(bn)
    g, E, K = m.geom, m.embed_len, hps.bn_vq_n_embed
    eng = m._ensure_engine(1)
    before = _state(eng)
    assert "emb" in before and (bn != "vqvae-ema" or len(before) == 4)
    eng.set_inputs(wav, mel, voice, jit)
    cond0, bias0 = (t.clone() for t in eng.conditioning())
    ind0, dist0 = eng.ind[:eng.Q].clone(), eng.min_dist[:eng.Q].clone()
    assert eng.codes_bad is None                                      # nothing of the decode side exists yet
    # encode: the codes conditioning() left, as a fresh tensor
    eng.ind.fill_(-3)
    codes, dist = m.encode(mel, return_dist=True)
    assert codes.shape == (1, E) and codes.dtype == torch.int64 and dist.shape == (1, E)
    assert torch.equal(codes.view(-1), ind0) and torch.equal(eng.ind[:eng.Q], ind0) and torch.equal(dist.view(-1), dist0)
    assert codes.data_ptr() != eng.ind.data_ptr() and 0 <= int(codes.min()) and int(codes.max()) < K
    assert torch.equal(m.encode(mel), codes)
    # codes -> conditioning: byte-equal to conditioning() (B = 1, same plans, only the writer of zq differs)
    eng.bn.code.tensor().fill_(7.0)
    eng.dec.cond.tensor().zero_()
    eng.dec.bias_bl.zero_()
    eng.ind.fill_(-3)
    cond1, bias1 = eng.codes_to_conditioning(codes)
    assert torch.equal(eng.ind[:eng.Q], ind0) and int(eng.codes_bad[0]) == 0
    assert torch.equal(_bits(cond1), _bits(cond0)) and torch.equal(_bits(bias1), _bits(bias0))
    assert torch.equal(eng.bn.code.tensor()[0, :, :hps.bn_n_out], eng.emb[ind0])
    # decode == sample, exactly (one replica, the same seed, the window given as the prime)
    T, o = g.dec_in_len, int(g.trim_dec_in[0])
    given = wav[:, o:o + T]
    ref = m.sample(wav, mel, voice, jit, seed=5)
    assert ref.shape == (2, T)
    out = m.decode(codes, voice, prime=given, seed=5)
    assert out.shape == (1, T) and out.dtype == torch.float32 and torch.equal(out, ref[1:])
    rf = m._sampler[1].g.rf()
    assert 0 < rf + 1 < T and torch.equal(out[:, :rf + 1], given[:, :rf + 1])
    # no prime: the forced positions hold the value silence encodes to
    quiet = m.decode(codes, voice, seed=5)
    assert float(quiet[:, :rf + 1].min()) == float(quiet[:, :rf + 1].max()) == 128.0 == float(m.zero_amplitude_code())
    assert 0 <= float(quiet.min()) and float(quiet.max()) < 256
    # nothing of the codebook and its statistics moved
    for n, t in _state(eng).items():
        assert torch.equal(_bits(t), _bits(before[n])), n
    # training goes on ...
    m.train()
    opt = optim.FusedAdam(m, lr=1e-4)
    opt.zero_grad()
    pred, target, loss = m.run(wav, mel, voice, jit)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and pred.shape == (1, 256, 95)
    assert all(bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    # ... but a loss computed before an encode() has lost its activations
    _, _, stale = m.run(wav, mel, voice, jit)
    m.encode(mel)
    with pytest.raises(L.AewError, match="overwrote the activations"):
        stale.backward()
    _, _, stale = m.run(wav, mel, voice, jit)
    m.decode(codes, voice, seed=1)
    with pytest.raises(L.AewError, match="overwrote the activations"):
        stale.backward()


def test_convert_one_window_into_three_voices():
    hps, m, (wav, mel, voice, jit) = _model("vqvae-ema")
    g, T, o = m.geom, m.dec_in_len, int(m.geom.trim_dec_in[0])
    voices = torch.tensor([0, 7, 23], device=DEV)
    out = m.convert(wav, mel, voices, seed=3)
    eng = m._engine
    assert eng.B == 3
    cond, bias = eng.dec.cond.tensor(), eng.dec.bias_bl[:3 * eng.dec.NL * 2 * eng.dec.Dp].view(3, -1)
    assert torch.equal(_bits(cond[1]), _bits(cond[0])) and torch.equal(_bits(cond[2]), _bits(cond[0]))
    assert not torch.equal(bias[0], bias[1]) and not torch.equal(bias[1], bias[2]) and not torch.equal(bias[0], bias[2])
    rf = m._sampler[1].g.rf()
    assert out.shape == (3, T) and out.dtype == torch.float32
    assert 0 <= float(out.min()) and float(out.max()) < 256 and torch.equal(out, out.round())
    assert torch.equal(out[:, :rf + 1], wav[:, o:o + rf + 1].expand(3, -1))
    assert torch.equal(m.convert(wav, mel, voices, seed=3), out)
    # voice_to (B,): the plain form equals decode(encode(mel), ...)
    one = m.convert(wav, mel, voices[1:2], seed=3)
    assert torch.equal(one, m.decode(m.encode(mel), voices[1:2], prime=wav[:, o:o + T], seed=3))
    with pytest.raises(L.AewError):
        m.convert(wav.expand(2, -1), mel.expand(2, -1, -1), voices)


def test_decode_refuses_codes_outside_the_codebook_before_the_sampler_starts():
    hps, m, (wav, mel, voice, jit) = _model("vqvae")
    K = hps.bn_vq_n_embed
    codes = m.encode(mel)
    good = m.decode(codes, voice, seed=2)
    smp, calls = m._sampler[1], []
    generate = smp.generate
    smp.generate = lambda *a, **k: (calls.append(1), generate(*a, **k))[1]
    bad = codes.clone()
    bad[0, 3] = K
    with pytest.raises(L.AewError, match=f"1 of the {codes.numel()} codes"):
        m.decode(bad, voice, seed=2)
    assert not calls and m._sampler[1] is smp
    eng = m._engine
    assert int(eng.codes_bad[0]) == 1 and not eng.bn.code.tensor()[0, 3].any()      # the row was zeroed, in bounds
    bad[0, 0] = -1
    with pytest.raises(L.AewError, match="2 of the"):
        m.decode(bad, voice, seed=2)
    assert not calls
    assert torch.equal(m.decode(codes, voice, seed=2), good) and len(calls) == 1
    with pytest.raises(L.AewError):
        m.decode(codes[:, :-1], voice)
    with pytest.raises(L.AewError):
        m.decode(codes, voice.expand(2))
