"""Whole-utterance conditioning and generation on the device: AEW_OP_CODE_TILE and AEW_OP_COND_STITCH alone, bit for bit
against their numpy restatements (tests/cond_utterance_emulator.py) with canaries around every destination; the seam -
model.utterance_conditioning() against TrainEngine.codes_to_conditioning() on hand-cut windows; the sampler over an
utterance-length conditioning against the same sampler over one window; model.decode_utterances() and
convert_utterances(); one batch replayed from a captured graph.

The model is tests/test_codes_gpu.py::_model with n_win_batch = 1000 (96 cannot tile): E = 11 codes per window, T = 1030
rows, S = 320 positions per code, trim0 = 0, hop h = 3 codes, L(n) = 320 n - 2172, o = 2235."""
import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, autoencoder_model as ae, codes as CD, config, geometry as G, optim
from tests import cond_utterance_emulator as CE
from tests.test_codes_gpu import _bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0x7777
K = 128
N_CODES = list(CE.CASES)                                 # 6, 7, 9, 10, 11, 12, 17
LENGTHS = [0, 68, 708, 1028, 1348, 1668, 3268]
VOICES = [3, 0, 17, 39, 8, 8, 21]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(kind, rec):
    CD._run(kind, rec, "conditioning op", torch.device(DEV))


def _pinned(tbl):
    host = torch.empty(tbl.nbytes, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = tbl.view(np.uint8).reshape(-1)
    return host


# ---- 4. the two ops alone ----------------------------------------------------------------------------------------------
# A synthetic geometry whose hop is an odd number of rows: E = 7, S = 5, T = 18, trim0 = 3 -> p = 1, lead 2, h = 3, hop
# 15; L(n) = 5 n - 9.  Code counts 1 (no row), 2 (one row), 5, 7, 12 -> 0 + 1 + 2 + 2 + 4 = 9 windows: at B = 5 two
# batches with one idle row.  pitch = 51 rows, so streams 1, 3 start at odd rows and every second window at an odd one.
SYN = dict(E=7, S=5, T=18, trim0=3)
SYN_CODES = [1, 2, 5, 7, 12]
SYN_B = 5


def _syn_plan():
    L_of = lambda n: max(5 * n - 9, 0)
    plan = CD.cond_tile_plan(SYN_CODES, SYN["E"], SYN["S"], SYN["T"], SYN["trim0"], SYN_B, L_of)
    assert (plan.p, plan.h, plan.pitch, plan.n_rows, len(plan.utt)) == (1, 3, 51, 9, 10)
    bases = np.concatenate([[0], np.cumsum(SYN_CODES)])[:-1]
    return plan, plan.table(bases, [4, 0, 2, 1, 3])


def _stitch_op(tbl_d, tbl_h, first, cond, cond_bs, Cp, cond_utt, n_streams, bias, bias_utt, bias_n):
    cs = L.CondStitch()
    cs.table, cs.table_host, cs.first_row, cs.B = tbl_d.data_ptr(), tbl_h.data_ptr(), first, SYN_B
    cs.cond, cs.cond_bs, cs.cond_pitch, cs.T, cs.Cp = cond.data_ptr() + 2 * 8 * Cp, cond_bs, Cp, SYN["T"], Cp
    cs.cond_utt, cs.n_dst = cond_utt.data_ptr(), n_streams * 51 * Cp
    cs.bias, cs.bias_utt, cs.bias_n, cs.n_streams = bias.data_ptr(), bias_utt.data_ptr(), bias_n, n_streams
    return cs


@pytest.mark.parametrize("Cp", [32, 128])
def test_code_tile_and_cond_stitch_equal_the_emulator_bit_for_bit(Cp):
    plan, tbl = _syn_plan()
    assert (tbl["dst_row"] % 2 == 1).any() and (tbl["utt"] < 0).sum() == 1 and tbl["utt"][-1] == -1
    E, T, n_streams, bias_n = SYN["E"], SYN["T"], len(SYN_CODES), 3 * 2 * 8
    rs = np.random.RandomState(Cp)
    codes = rs.randint(1, K, sum(SYN_CODES)).astype(np.int64)
    codes[[3, 9, 20]] = [K, -1, np.iinfo(np.int64).max]                   # outside the codebook: written as 0, counted
    codes_d, tbl_d, tbl_h = _dev(codes), _dev(tbl.view(np.uint8).reshape(-1)), _pinned(tbl)
    ind = torch.full((SYN_B * E + 64,), -9, dtype=torch.int64, device=DEV)
    voice = torch.full((SYN_B + 64,), -9, dtype=torch.int64, device=DEV)
    bad = torch.zeros(4, dtype=torch.int32, device=DEV)
    T_g = T + 16                                                           # guard rows around every batch row, as dec.cond has
    cond = rs.randint(0, 1 << 16, (SYN_B, T_g, Cp)).astype(np.uint16)
    bias = rs.standard_normal((SYN_B, bias_n)).astype(np.float32)
    cond_d, bias_d = _dev(cond.view(np.int16)), _dev(bias)
    cond_utt = torch.full((n_streams * 51 * Cp + 64,), CANARY, dtype=torch.int16, device=DEV)
    bias_utt = torch.full((n_streams * bias_n + 64,), -7.0, dtype=torch.float32, device=DEV)
    want_cond = np.full((n_streams, 51, Cp), CANARY, np.uint16)
    want_bias = np.full((n_streams, bias_n), -7.0, np.float32)
    want_bad = 0
    for first in range(0, len(tbl), SYN_B):
        ct = L.CodeTile()
        ct.table, ct.table_host, ct.first_row, ct.B = tbl_d.data_ptr(), tbl_h.data_ptr(), first, SYN_B
        ct.codes, ct.n_codes, ct.ind, ct.in_voice, ct.bad = codes_d.data_ptr(), codes.size, ind.data_ptr(), voice.data_ptr(), bad.data_ptr()
        ct.E, ct.K, ct.n_voice = E, K, 5
        ind.fill_(-9)
        voice.fill_(-9)
        _run(L.OP_CODE_TILE, ct)
        w_ind, w_voice, n_bad = CE.code_tile(tbl, first, SYN_B, codes, E, K)
        want_bad += n_bad
        got_i, got_v = ind.cpu().numpy(), voice.cpu().numpy()
        assert got_i[:SYN_B * E].tobytes() == w_ind.tobytes() and (got_i[SYN_B * E:] == -9).all(), first
        assert got_v[:SYN_B].tobytes() == w_voice.tobytes() and (got_v[SYN_B:] == -9).all(), first
        assert bad.cpu().tolist() == [want_bad, 0, 0, 0]
        _run(L.OP_COND_STITCH, _stitch_op(tbl_d, tbl_h, first, cond_d, T_g * Cp, Cp, cond_utt, n_streams, bias_d, bias_utt, bias_n))
        CE.cond_stitch(tbl, first, SYN_B, cond[:, 8:8 + T], want_cond, bias, want_bias)
        got_c, got_b = cond_utt.cpu().numpy().view(np.uint16), bias_utt.cpu().numpy()
        assert got_c[:want_cond.size].tobytes() == want_cond.tobytes(), first      # every row outside the owned ranges: canary
        assert (got_c[want_cond.size:] == CANARY).all()
        assert got_b[:want_bias.size].tobytes() == want_bias.tobytes() and (got_b[want_bias.size:] == -7.0).all(), first
    assert want_bad >= 3                                                   # (overlapping windows see a bad code twice)
    for u, n in enumerate(plan.lengths):                                   # all of every utterance arrived, nothing behind it
        assert not (want_cond[u, :n] == CANARY).all(axis=1).any() and (want_cond[u, n:] == CANARY).all()
    assert (want_bias[0] == -7.0).all() and not (want_bias[1:] == -7.0).any()      # (utterance 0 has no window)


def test_malformed_records_are_refused_with_nothing_written():
    plan, good = _syn_plan()
    E, T, Cp, n_streams, bias_n = SYN["E"], SYN["T"], 32, len(SYN_CODES), 48
    codes = torch.ones(sum(SYN_CODES), dtype=torch.int64, device=DEV)
    ind = torch.full((SYN_B * E,), -9, dtype=torch.int64, device=DEV)
    voice = torch.full((SYN_B + 1,), -9, dtype=torch.int64, device=DEV)
    bad = torch.zeros(4, dtype=torch.int32, device=DEV)
    cond = torch.zeros(SYN_B * (T + 16) * Cp, dtype=torch.int16, device=DEV)
    bias = torch.zeros(SYN_B * bias_n, device=DEV)
    cond_utt = torch.full((n_streams * 51 * Cp,), CANARY, dtype=torch.int16, device=DEV)
    bias_utt = torch.full((n_streams * bias_n,), -7.0, device=DEV)

    def ops(tbl):
        d, h = _dev(tbl.view(np.uint8).reshape(-1)), _pinned(tbl)
        ct = L.CodeTile()
        ct.table, ct.table_host, ct.first_row, ct.B = d.data_ptr(), h.data_ptr(), 0, SYN_B
        ct.codes, ct.n_codes, ct.ind, ct.in_voice, ct.bad = codes.data_ptr(), codes.numel(), ind.data_ptr(), voice.data_ptr(), bad.data_ptr()
        ct.E, ct.K, ct.n_voice = E, K, 5
        return ct, _stitch_op(d, h, 0, cond, (T + 16) * Cp, Cp, cond_utt, n_streams, bias, bias_utt, bias_n), (d, h)

    live = int(np.flatnonzero(good["utt"][:SYN_B] >= 0)[-1])
    for field, value, kind in (("hi", E + 1, L.OP_CODE_TILE), ("lo", -1, L.OP_CODE_TILE), ("code0", codes.numel(), L.OP_CODE_TILE),
                               ("voice", 5, L.OP_CODE_TILE), ("src_row", T, L.OP_COND_STITCH), ("n_rows", T + 1, L.OP_COND_STITCH),
                               ("dst_row", 50, L.OP_COND_STITCH), ("stream", n_streams, L.OP_COND_STITCH),
                               ("pitch", 10, L.OP_COND_STITCH)):
        tbl = good.copy()
        tbl[field][live] = value
        ct, cs, keep = ops(tbl)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(kind, ct if kind == L.OP_CODE_TILE else cs)
    for field in ("table", "table_host", "codes", "ind", "in_voice", "bad"):
        ct, cs, keep = ops(good)
        setattr(ct, field, None)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(L.OP_CODE_TILE, ct)
    for field, value in (("cond", None), ("cond_utt", None), ("bias_utt", None), ("B", 0), ("Cp", 36), ("bias_n", 6),
                         ("n_dst", 4 * 51 * Cp - 1)):                    # (the batch's last stream is 3)
        ct, cs, keep = ops(good)
        setattr(cs, field, value)
        with pytest.raises(L.AewError, match="rc=-1"):
            _run(L.OP_COND_STITCH, cs)
    for kind, field, off in ((L.OP_CODE_TILE, "in_voice", 8), (L.OP_CODE_TILE, "bad", 2), (L.OP_COND_STITCH, "cond_utt", 8),
                             (L.OP_COND_STITCH, "bias_utt", 4), (L.OP_COND_STITCH, "cond", 2)):
        ct, cs, keep = ops(good)
        rec = ct if kind == L.OP_CODE_TILE else cs
        setattr(rec, field, getattr(rec, field) + off)
        with pytest.raises(L.AewError, match="rc=-3"):
            _run(kind, rec)
    torch.cuda.synchronize()
    assert (ind == -9).all() and (voice == -9).all() and not bad.any()
    assert (cond_utt == CANARY).all() and (bias_utt == -7.0).all()


# ---- the model -----------------------------------------------------------------------------------------------------------
def _model(bn="vqvae-ema"):
    """tests/test_codes_gpu.py::_model with a window the conditioning can tile (n_win_batch = 1000)."""
    hps = config.make_hps(bn, n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64,
                          bn_n_out=16, bn_vq_n_embed=K, n_win_batch=1000, n_blocks=2, n_block_layers=4)
    torch.manual_seed(0)
    m = ae.AutoEncoder(hps, n_mel=39).to(DEV)
    g = m.geom
    gen = torch.Generator().manual_seed(1)
    args = (torch.randint(0, 256, (1, g.enc_in_len), generator=gen).float().to(DEV),
            torch.randn(1, 39, g.mel_len, generator=gen).to(DEV), torch.randint(0, 40, (1,), generator=gen).to(DEV),
            torch.arange(g.embed_len).repeat(1, 1).to(DEV))
    return hps, m, args


def _utterances(seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in N_CODES]


def _state(eng):
    return {n: getattr(eng, n).clone() for n in ("emb", "ema_numer", "ema_denom", "ind_hist") if hasattr(eng, n)}


_SHARED = {}


@pytest.fixture(scope="module")
def shared():
    """One model, the seven utterances and their conditioning at batch = 3, computed once for the tests that only read."""
    if not _SHARED:
        hps, m, args = _model()
        utts = _utterances()
        cond, bias, lengths = m.utterance_conditioning(utts, voice=VOICES, batch=3)
        torch.cuda.synchronize()
        _SHARED.update(hps=hps, m=m, args=args, utts=utts, cond=cond, bias=bias, lengths=lengths)
    return _SHARED


# ---- 5. the seam ---------------------------------------------------------------------------------------------------------
def test_stitched_conditioning_equals_codes_to_conditioning_on_every_window(shared):
    m, utts, cond_utt, bias_utt, lengths = (shared[k] for k in ("m", "utts", "cond", "bias", "lengths"))
    E, S, T, trim0, p, h, L_of = G.conditioning_geometry(m.geom)
    assert (E, S, T, trim0, p, h) == (11, 320, 1030, 0, 0, 3) and G.conditioning_geometry(m.geom).o == 2235
    assert lengths.tolist() == LENGTHS == [L_of(n) for n in N_CODES]
    eng = m._engine
    assert eng.B == 3 and cond_utt.shape == (16, 3268, eng.dec.Cp) and bias_utt.shape == (16, eng.dec.NL, 2 * eng.dec.Dp)
    assert cond_utt.dtype == torch.bfloat16 and bias_utt.dtype == torch.float32
    for u, n in enumerate(LENGTHS):                                       # rows behind L(N_u), and the streams behind U: zero
        assert not _bits(cond_utt[u, n:]).any(), u
        assert n == 0 or _bits(cond_utt[u, :n]).any()
    assert not _bits(cond_utt[7:]).any() and not bias_utt[7:].any() and not bias_utt[0].any()
    # every window start that exists, and - for the utterances shorter than a window - the one window padded with code 0
    cases = []
    for u, N in enumerate(N_CODES):
        starts = sorted({c for c in (0, 1, h - 1, h, N - E) if 0 <= c and c + E <= N}) if N >= E else ([0] if LENGTHS[u] else [])
        cases += [(u, c0) for c0 in starts]
    assert [c for c in cases if c[0] == 6] == [(6, 0), (6, 1), (6, 2), (6, 3), (6, 6)] and len(cases) == 11
    eng.in_jitter.copy_(torch.arange(E, device=DEV).expand(3, -1))
    for at in range(0, len(cases), 3):
        chunk = (cases[at:at + 3] * 3)[:3]
        wins = torch.zeros(3, E, dtype=torch.int64, device=DEV)
        for b, (u, c0) in enumerate(chunk):
            part = utts[u][c0:c0 + E]
            wins[b, :part.numel()] = part
            eng.in_voice[b] = VOICES[u]
        cond, bias = eng.codes_to_conditioning(wins)
        assert int(eng.codes_bad[0]) == 0
        for b, (u, c0) in enumerate(chunk):
            q0 = c0 * S + trim0
            n = min(T, LENGTHS[u] - q0)
            assert n > 0
            assert torch.equal(_bits(cond[b, :n]), _bits(cond_utt[u, q0:q0 + n])), (u, c0)
            assert torch.equal(_bits(bias[b]), _bits(bias_utt[u])), (u, c0)
    # an UtteranceCodes carries its voices along; the default batch is the live engine's
    uc = CD.UtteranceCodes(torch.cat(utts), torch.tensor(np.concatenate([[0], np.cumsum(N_CODES)])), voice=torch.tensor(VOICES))
    cond2, bias2, len2 = m.utterance_conditioning(uc)
    assert m._engine is eng and len2.tolist() == LENGTHS
    assert torch.equal(_bits(cond2), _bits(cond_utt)) and torch.equal(_bits(bias2), _bits(bias_utt))


# ---- 6. the sampler at utterance length ------------------------------------------------------------------------------------
def test_sampler_over_an_utterance_equals_the_sampler_over_one_window(shared):
    """Every position forced; the logits of a position depend on the previous rf inputs and its cond row only, so from
    rf positions past the window's start on, the run over the 17-code utterance's 3268 rows and the run over its window
    at c0 = 1 (rows 320 .. 1350) are expected to agree bit for bit."""
    m, utts, cond_utt, bias_utt = (shared[k] for k in ("m", "utts", "cond", "bias"))
    E, S, T, trim0, p, h, L_of = G.conditioning_geometry(m.geom)
    eng = m._ensure_engine(3)
    smp = m._engine_sampler(eng)
    rf, Ln, u, c0 = smp.g.rf(), LENGTHS[6], 6, 1
    gen = torch.Generator().manual_seed(4)
    forced = torch.randint(0, 256, (1, Ln), generator=gen).to(torch.int32).to(DEV).expand(16, -1).contiguous()
    rows = torch.full((16,), u, device=DEV)
    wav, logits = smp.generate(cond_utt[rows].contiguous(), bias_utt[rows].contiguous(), forced, seed=1, want_logits=True)
    assert torch.equal(wav, forced)
    eng.in_jitter.copy_(torch.arange(E, device=DEV).expand(3, -1))
    eng.in_voice.fill_(VOICES[u])
    cond, bias = eng.codes_to_conditioning(utts[u][c0:c0 + E].repeat(3))
    q0 = c0 * S + trim0
    zero = torch.zeros(16, dtype=torch.long, device=DEV)
    wav_w, logits_w = smp.generate(cond[zero].contiguous(), bias[zero].contiguous(), forced[:, q0:q0 + T].contiguous(), seed=1,
                                   want_logits=True)
    got, want = logits_w[0, rf:], logits[0, q0 + rf:q0 + T]
    err = (got - want).abs().max().item()
    print(f"window vs utterance logits: max abs difference {err:.3e} over {got.shape[0]} positions (scale {want.abs().max().item():.2f})")
    assert torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(logits[3]), _bits(logits[0]))                 # (and the streams of one batch agree)


# ---- 7. generation -----------------------------------------------------------------------------------------------------------
def test_decode_utterances_generates_every_length_reproducibly():
    hps, m, (wav1, mel1, voice1, jit1) = _model()
    utts = _utterances()
    eng = m._ensure_engine(3)
    before = _state(eng)
    assert len(before) == 4
    out = m.decode_utterances(utts, voice=VOICES, seed=5, batch=3)
    assert m._engine is eng
    rf = m._sampler[1].g.rf()
    assert rf == 30 and [o.numel() for o in out] == LENGTHS
    for o, n in zip(out, LENGTHS):
        assert o.dtype == torch.float32 and o.device.type == "cuda" and o.shape == (n,)
        assert torch.equal(o, o.round()) and (n == 0 or (0 <= float(o.min()) and float(o.max()) < 256))
        assert (o[:min(rf + 1, n)] == 128.0).all()                        # no prime: the value silence encodes to
    assert float(m.zero_amplitude_code()) == 128.0 and any(len(o.unique()) > 8 for o in out)
    again = m.decode_utterances(utts, voice=VOICES, seed=5, batch=3)
    assert all(torch.equal(a, b) for a, b in zip(again, out))             # the same seed: bit-equal
    other = m.decode_utterances(utts, voice=VOICES, seed=6, batch=3)
    assert not torch.equal(other[6], out[6])
    # a prime: the first rf + 1 values (clipped to the length) are the prime's; n_prime moves the boundary
    gen = torch.Generator().manual_seed(2)
    prime = [torch.randint(0, 256, (max(n, 1),), generator=gen).float().to(DEV) for n in LENGTHS]
    primed = m.decode_utterances(utts, voice=VOICES, prime=prime, seed=5, batch=3)
    for o, pr, n in zip(primed, prime, LENGTHS):
        k = min(rf + 1, n)
        assert o.numel() == n and torch.equal(o[:k], pr[:k])
    assert torch.equal(m.decode_utterances(utts[6:], voice=VOICES[6:], prime=prime[6:], n_prime=100, seed=5)[0][:100], prime[6][:100])
    # [A, B] and [A] alone give the same A when A is the longest: padding and neighbouring streams do not leak
    a_b = m.decode_utterances([utts[6], utts[4]], voice=[VOICES[6], VOICES[4]], seed=9, batch=3)
    a = m.decode_utterances([utts[6]], voice=[VOICES[6]], seed=9, batch=3)
    assert torch.equal(a_b[0], a[0]) and a_b[1].numel() == LENGTHS[4]
    b_a = m.decode_utterances([utts[4], utts[6]], voice=[VOICES[4], VOICES[6]], seed=9, batch=3)      # input order comes back
    assert torch.equal(b_a[1], a[0]) and torch.equal(b_a[0], a_b[1])
    # an UtteranceCodes with its voices; nothing of the codebook and its statistics moved
    uc = CD.UtteranceCodes(torch.cat(utts), torch.tensor(np.concatenate([[0], np.cumsum(N_CODES)])), voice=torch.tensor(VOICES))
    assert all(torch.equal(x, y) for x, y in zip(m.decode_utterances(uc, seed=5, batch=3), out))
    assert m._engine is eng
    for n, t in _state(eng).items():
        assert torch.equal(_bits(t), _bits(before[n])), n
    # a code equal to K raises before the sampler starts
    smp, calls = m._sampler[1], []
    generate = smp.generate
    smp.generate = lambda *a_, **k_: (calls.append(1), generate(*a_, **k_))[1]
    bad = [u.clone() for u in utts]
    bad[3][4] = K
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.decode_utterances(bad, voice=VOICES, seed=5, batch=3)
    bad[3][4], bad[0][1] = 0, -1                                          # (in an utterance too short to take a stream, too)
    with pytest.raises(L.AewError, match="outside the codebook"):
        m.decode_utterances(bad, voice=VOICES, seed=5, batch=3)
    assert not calls
    smp.generate = generate
    with pytest.raises(L.AewError):
        m.decode_utterances(utts, voice=VOICES[:-1])
    with pytest.raises(L.AewError):
        m.decode_utterances(utts, voice=[40] + VOICES[1:])
    with pytest.raises(L.AewError):
        m.decode_utterances(utts)                                         # no voice anywhere
    # training goes on ...
    m.train()
    opt = optim.FusedAdam(m, lr=1e-4)
    opt.zero_grad()
    pred, target, loss = m.run(wav1, mel1, voice1, jit1)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and pred.shape == (1, 256, 999)
    assert all(bool(torch.isfinite(q).all()) and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    # ... but a loss computed before the call has lost its activations
    _, _, stale = m.run(wav1, mel1, voice1, jit1)
    m.decode_utterances(utts[1:2], voice=VOICES[1:2], seed=1)
    with pytest.raises(L.AewError, match="overwrote the activations"):
        stale.backward()


def test_models_that_cannot_tile_or_have_no_codes_are_refused():
    small = dict(n_res=64, n_dil=64, n_skp=64, n_post=64, n_lc_out=32, enc_n_out=64, bn_n_out=16, n_blocks=2, n_block_layers=4)
    codes = [torch.zeros(12, dtype=torch.int64, device=DEV)]
    m = ae.AutoEncoder(config.make_hps("vqvae", bn_vq_n_embed=K, n_win_batch=96, **small), n_mel=39).to(DEV)
    with pytest.raises(L.AewError, match="n_win_batch >= 290"):
        m.decode_utterances(codes, voice=[0])
    m = ae.AutoEncoder(config.make_hps("ae", n_win_batch=1000, **small), n_mel=39).to(DEV)
    with pytest.raises(L.AewError, match="discrete codes"):
        m.decode_utterances(codes, voice=[0])
    m = ae.AutoEncoder(config.make_hps("vqvae", bn_vq_n_embed=K, n_win_batch=1000, **small), n_mel=39, take_compat=True).to(DEV)
    with pytest.raises(L.AewError, match="take_compat"):
        m.utterance_conditioning(codes, voice=[0])


# ---- 8. conversion -----------------------------------------------------------------------------------------------------------
def test_convert_utterances_is_encode_wavs_then_decode_utterances(shared):
    m = shared["m"]
    o = G.conditioning_geometry(m.geom).o
    gen = torch.Generator().manual_seed(8)
    wav = torch.randint(0, 256, (9000,), generator=gen).float().to(DEV)
    uc = m.encode_wavs([wav], batch=3)
    n = G.conditioning_geometry(m.geom).L(uc.row(0).numel())
    assert 0 < n <= wav.numel() - o
    got = m.convert_utterances([wav], [7], seed=3, batch=3)
    want = m.decode_utterances(uc, [7], prime=[wav[o:]], seed=3, batch=3)
    assert len(got) == 1 and got[0].shape == (n,) and torch.equal(got[0], want[0])
    rf = m._sampler[1].g.rf()
    assert torch.equal(got[0][:rf + 1], wav[o:o + rf + 1])
    # one utterance into three voices: three streams that share the conditioning bits and differ in bias
    voices = torch.tensor([0, 7, 23])
    three = m.convert_utterances([wav], voices, seed=3, batch=3)
    assert len(three) == 3 and all(t.shape == (n,) and torch.equal(t[:rf + 1], wav[o:o + rf + 1]) for t in three)
    assert all(torch.equal(a, b) for a, b in zip(m.convert_utterances([wav], voices, seed=3, batch=3), three))
    cond, bias, lengths = m.utterance_conditioning([uc.row(0)] * 3, voice=voices, batch=3)
    assert lengths.tolist() == [n] * 3
    assert torch.equal(_bits(cond[1]), _bits(cond[0])) and torch.equal(_bits(cond[2]), _bits(cond[0])) and _bits(cond[0]).any()
    assert not torch.equal(bias[0], bias[1]) and not torch.equal(bias[1], bias[2]) and not torch.equal(bias[0], bias[2])
    with pytest.raises(L.AewError):
        m.convert_utterances([wav, wav], voices)


# ---- one batch from a captured graph -----------------------------------------------------------------------------------------
def test_a_captured_batch_tracks_new_input(shared):
    m = shared["m"]
    eng = m._ensure_engine(3)
    cg = G.conditioning_geometry(m.geom)
    n_codes = [12, 9]                                                     # two windows + one: one batch of three rows
    plan = CD.cond_tile_plan(n_codes, cg.E, cg.S, cg.T, cg.trim0, 3, cg.L)
    assert plan.n_batches == 1 and plan.n_rows == 3
    tbl = plan.table([0, 12], [5, 9])
    host = _pinned(tbl)
    dev = host.to(DEV)
    d = eng.dec
    flat = torch.zeros(21, dtype=torch.int64, device=DEV)
    cond = torch.zeros(16, plan.pitch, d.Cp, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(16, d.NL, 2 * d.Dp, device=DEV)
    p = eng.conditioning_batch_plan(flat, dev, host, 0, cond, bias)
    assert p.labels[0] == "code.tile" and p.labels[1] == "code.lookup" and p.labels[-1] == "cond.stitch" and len(p.ops) > 4
    assert "vq.ema" not in p.labels and "diagnostics (codebook)" not in p.labels
    gen = torch.Generator().manual_seed(9)
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(3):                                                  # capture + first launch, then two replays
        utts = [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in n_codes]
        flat.copy_(torch.cat(utts))
        cond.zero_()
        bias.zero_()
        eng.codes_bad.zero_()
        p.run_graph(st)
        assert p._graph is not None
        got_c, got_b = cond.clone(), bias.clone()
        want_c, want_b, _ = m.utterance_conditioning(utts, voice=[5, 9], batch=3)
        assert torch.equal(_bits(got_c), _bits(want_c)) and torch.equal(_bits(got_b), _bits(want_b)), rep
    # the table is read on the device at every replay: with the second utterance's row made idle its stream stays zero
    idle = tbl.copy()
    idle[2] = np.zeros(1, tbl.dtype)[0]
    idle["utt"][2] = -1
    dev.copy_(_dev(idle.view(np.uint8).reshape(-1)))
    cond.zero_()
    bias.zero_()
    p.run_graph(st)
    assert torch.equal(_bits(cond[0]), _bits(want_c[0])) and not _bits(cond[1]).any() and not bias[1].any()
    # ... and a code outside the codebook met in a replay is counted, not followed
    dev.copy_(_dev(tbl.view(np.uint8).reshape(-1)))
    flat[3] = K
    eng.codes_bad.zero_()
    p.run_graph(st)
    assert int(eng.codes_bad[0]) > 0
    p.invalidate_graph()
