"""Draw controls of the sampler on the MI355X (csrc/aew_sampler.hip, the DRAW instantiation of the persistent kernel;
ae_wavenet_amd/sampler.py: Draw, draw_table, generate(draw=...); surface.py: the draw argument of the sampling calls).

Every check of a drawn value is made from the kernel's OWN recorded logits (want_logits=True) with the numpy restatement
of the rule, tests/sampler_draw_emulator.py: greedy / top_k = 1 picks are the first value in the order, top-k picks lie in
the exact K-set (logit bits only), and every pick whose nucleus set fp32 can decide satisfies the inverse-CDF interval
check of tests/test_sampler.py (d) over the emulator's kept set.  Steps the emulator calls ambiguous are left out; their
share is bounded.  Every generate() here keeps the default bounded spin_max."""
import numpy as np
import pytest
import torch

from ae_wavenet_amd import codes as CD, config, geometry as G, sampler as S
from ae_wavenet_amd.sampler import Draw, draw_table
from tests import sampler_draw_emulator as DE
from tests.test_sampler import DEV, RNG_STEP, TINY, _dec_wav, _engine

pytestmark = pytest.mark.gpu

RECORDS = [Draw(), Draw(0.7), Draw(1.5), Draw.greedy(), Draw(top_k=1), Draw(top_k=20), Draw(top_p=0.9), Draw(0.8, 40, 0.5)]
_CACHE = {}


def _tiny(seed=7):
    """(sampler, cond, bias, forced, n_prime) of the TINY decoder: 32 streams, T = 54, 39 drawn positions per stream."""
    if seed not in _CACHE:
        hps, eng, wts, emb, inp = _engine(32, 40, seed, **TINY)
        smp = S.from_engine(eng)
        cond, bias = S.engine_conditioning(eng)
        given = _dec_wav(eng, inp).to(DEV)
        n_prime = smp.g.rf() + 1
        forced = given.clone()
        forced[:, n_prime:] = -1
        assert forced.shape == (32, 54) and forced.shape[1] - n_prime == 39
        _CACHE[seed] = (eng, smp, cond, bias, forced, n_prime)
    return _CACHE[seed][1:]


def _check_draws(wav, logits, recs, seed, n_prime):
    """The per-position checks; returns (ambiguous steps, steps of streams with a nucleus)."""
    from oracle import jitter_rng
    lg, wv = logits.cpu().numpy(), wav.cpu().numpy()
    n, T = wv.shape
    Q = lg.shape[2]
    assert wv.min() >= 0 and wv.max() < Q
    u = jitter_rng.uniform(seed, RNG_STEP, n, T).astype(np.float32)
    amb = nuc = 0
    for s in range(n):
        inv, k, p, fl = recs[s].record()
        for t in range(n_prime - 1, T - 1):
            l, v = lg[s, t], int(wv[s, t + 1])
            if (fl & 1) or k == 1:
                assert v == DE.order(l)[0], (s, t, v)
            if 0 < k < Q:
                assert DE.k_set(l, k)[v], (s, t, v, k)
            _, keep, a = DE.draw(l, u[s, t + 1], inv, k, p, bool(fl & 1))
            if p < 1 and not (fl & 1):
                nuc += 1
                amb += a
            if not a:
                assert DE.interval_ok(l, u[s, t + 1], v, keep, inv), (s, t, v, recs[s])
    return amb, nuc


def _mixed_checks(smp, cond, bias, forced, n_prime, recs, seed):
    n = forced.shape[0]
    wav, logits = smp.generate(cond, bias, forced, seed=seed, want_logits=True, draw=recs)
    assert smp.last["draw"] and torch.equal(wav[:, :n_prime], forced[:, :n_prime])
    amb, nuc = _check_draws(wav, logits, recs, seed, n_prime)
    print(f"{n} streams, {wav.shape[1] - n_prime} drawn positions each: {amb} ambiguous of {nuc} nucleus steps")
    assert nuc > 0 and amb <= 0.05 * nuc
    # teacher-forcing the generated sequence reproduces the logits bit for bit; two runs are bit-equal
    _, logits_tf = smp.generate(cond, bias, wav.clone(), seed=0, want_logits=True, draw=recs)
    assert torch.equal(logits, logits_tf)
    wav2, logits2 = smp.generate(cond, bias, forced, seed=seed, want_logits=True, draw=draw_table(recs, n).to(DEV))
    assert torch.equal(wav, wav2) and torch.equal(logits, logits2)
    # streams are independent: other records for the OTHER streams leave the neutral streams' bits alone - and those
    # are the bits of the run without a table
    neutral = [s for s in range(n) if recs[s].is_neutral()]
    other = [recs[s] if recs[s].is_neutral() else Draw(0.9, 3, 0.7) for s in range(n)]
    wav3, _ = smp.generate(cond, bias, forced, seed=seed, draw=other)
    plain, _ = smp.generate(cond, bias, forced, seed=seed)
    assert not smp.last["draw"]
    assert len(neutral) >= 2 and torch.equal(wav3[neutral], wav[neutral]) and torch.equal(plain[neutral], wav[neutral])
    assert not torch.equal(wav3, wav) and not torch.equal(plain, wav)
    return wav


# ---- 1 -------------------------------------------------------------------------------------------------------------------
def test_neutral_table_equals_no_table():
    smp, cond, bias, forced, n_prime = _tiny()
    for seed in (1234, 99):
        wav, logits = smp.generate(cond, bias, forced, seed=seed, want_logits=True)
        assert not smp.last["draw"]
        for table in (Draw(), [Draw()] * 32, draw_table(Draw(), 32)):
            wav_n, logits_n = smp.generate(cond, bias, forced, seed=seed, want_logits=True, draw=table)
            assert smp.last["draw"]                                 # the DRAW instantiation ran
            assert torch.equal(wav_n, wav) and torch.equal(logits_n, logits)
        assert len(wav[:, n_prime:].unique()) > 8


# ---- 2, 3 ----------------------------------------------------------------------------------------------------------------
def test_mixed_records_in_one_wave():
    smp, cond, bias, forced, n_prime = _tiny()
    recs = [RECORDS[s % 8] for s in range(32)]                       # each SAMPLE wave (4 streams) holds 4 different records
    _mixed_checks(smp, cond, bias, forced, n_prime, recs, seed=1234)


def test_uniform_waves():
    smp, cond, bias, forced, n_prime = _tiny()
    recs = [RECORDS[(s // 4) % 8] for s in range(32)]                # four equal records per wave
    _mixed_checks(smp, cond, bias, forced, n_prime, recs, seed=77)


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def test_tie_rule_on_the_device():
    """post2.weight = 0, post2.bias[i] = i % 7: the logits of every step are exactly those biases, with 36 exact ties at the
    maximum (6, 13, 20, ...)."""
    eng = _engine(32, 40, 7, **TINY)[1]
    pre = eng.dec.pre
    assert eng.ps.has(pre + "post2.bias")
    eng.ps.view(pre + "post2.weight").zero_()
    eng.ps.view(pre + "post2.bias").copy_((torch.arange(256) % 7).float())
    smp = S.from_engine(eng)
    cond, bias = S.engine_conditioning(eng)
    n_prime = smp.g.rf() + 1
    forced = torch.full((32, 54), -1, dtype=torch.int32, device=DEV)
    forced[:, :n_prime] = 128
    recs = [(Draw(top_k=5), Draw.greedy(), Draw(top_p=0.01), Draw(1.3, 5, 1.0))[s % 4] for s in range(32)]
    wav, logits = smp.generate(cond, bias, forced, seed=5, want_logits=True, draw=recs)
    want = (torch.arange(256, device=DEV) % 7).float()
    assert torch.equal(logits, want.expand_as(logits))
    drawn = wav[:, n_prime:].cpu().numpy()
    for s in range(32):
        if s % 4 in (0, 3):
            assert set(drawn[s].tolist()) <= {6, 13, 20, 27, 34}, (s, sorted(set(drawn[s].tolist())))
        else:
            assert (drawn[s] == 6).all(), (s, drawn[s])
    assert len(np.unique(drawn[0::4])) == 5                          # 8 streams x 39 draws over 5 equal weights: all occur


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_fewer_than_16_values_per_lane():
    """n_quant = 64: 4 logits per lane, the 8-byte load path; a synthetic sampler (no engine), 16 streams, T = 64."""
    smp, gen = _synthetic(3.0, n_quant=64, n_res=40, n_dil=16, n_skp=20, n_post=12, n_lc_out=8, n_global_embed=4, n_speakers=5,
                          n_blocks=2, n_block_layers=3)
    g, n, T = smp.g, 16, 64
    assert g.Q == 64
    cond = (torch.randn(n, T, g.Ck, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(n, g.NL, g.n_pairs * 32, generator=gen) * 0.1).to(DEV)
    forced = torch.full((n, T), -1, dtype=torch.int32)
    forced[:, 0] = 32
    recs = [RECORDS[s % 8] for s in range(n)]
    wav = _mixed_checks(smp, cond, bias, forced.to(DEV), 1, recs, seed=11)
    assert int(wav.max()) < 64


def _synthetic(gain, **over):
    """A Sampler over random weights, built as tools/bench_sampler.py builds one (no engine)."""
    from ae_wavenet_amd.engine import ParamStore, decoder_param_specs
    from ae_wavenet_amd.plan import Workspace
    hps = config.make_hps("vqvae-ema", **over)
    ps = ParamStore(Workspace(DEV), decoder_param_specs(hps, hps.bn_n_out, "decoder."))
    gen = torch.Generator().manual_seed(0)
    for k in ps.names():
        t = torch.empty(ps.shape[k])
        if len(ps.shape[k]) >= 2:
            torch.nn.init.xavier_uniform_(t, generator=gen, gain=gain)
        else:
            t.uniform_(-0.5, 0.5, generator=gen)
        ps.view(k).copy_(t)
    return S.Sampler(hps, ps, "decoder.", DEV), gen


def test_wide_residual_instantiation():
    """n_res = 512 takes the kernel's KR = 16 instantiations (30-layer / 512-channel decoders): every draw of a run with
    mixed records, and of a run with the neutral table, is the rule's pick from that run's own logits."""
    smp, gen = _synthetic(1.5, n_res=512, n_dil=16, n_skp=32, n_post=32, n_lc_out=8, n_global_embed=4, n_speakers=5,
                          n_blocks=1, n_block_layers=3)
    g, n, T = smp.g, 16, 40
    assert g.kr_max == 16 and g.Q == 256
    cond = (torch.randn(n, T, g.Ck, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(n, g.NL, g.n_pairs * 32, generator=gen) * 0.1).to(DEV)
    forced = torch.full((n, T), -1, dtype=torch.int32)
    forced[:, 0] = 128
    forced = forced.to(DEV)
    recs = [RECORDS[s % 8] for s in range(n)]
    wav, logits = smp.generate(cond, bias, forced, seed=3, want_logits=True, draw=recs)
    assert smp.last["draw"] and torch.equal(wav[:, 0], forced[:, 0])
    amb, nuc = _check_draws(wav, logits, recs, 3, 1)
    assert nuc > 0 and amb <= 0.05 * nuc
    wav_n, logits_n = smp.generate(cond, bias, forced, seed=3, want_logits=True, draw=Draw())
    _check_draws(wav_n, logits_n, [Draw()] * n, 3, 1)


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_out_of_range_controls_mean_off():
    smp, cond, bias, forced, n_prime = _tiny()
    wav, logits = smp.generate(cond, bias, forced, seed=1234, want_logits=True)
    raw = np.zeros(32, S.DRAW_DTYPE)
    raw["inv_temp"], raw["top_p"] = 1.0, 2.0
    raw["top_k"] = [(-3, 10 ** 6)[s % 2] for s in range(32)]
    table = torch.from_numpy(raw.view("<i4").reshape(32, 4).copy())
    wav_r, logits_r = smp.generate(cond, bias, forced, seed=1234, want_logits=True, draw=table)
    assert smp.last["draw"] and torch.equal(wav_r, wav) and torch.equal(logits_r, logits)


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def test_surface_draw_argument():
    from tests.test_cond_utterance_gpu import K, _model
    hps, m, (wav1, mel1, voice1, jit1) = _model()
    gen = torch.Generator().manual_seed(3)
    E = m.embed_len
    codes = torch.randint(0, K, (3, E), generator=gen).to(DEV)
    voice = torch.tensor([1, 7, 30], device=DEV)
    plain = m.decode(codes, voice, seed=5)
    assert torch.equal(m.decode(codes, voice, seed=5, draw=None), plain)
    assert torch.equal(m.decode(codes, voice, seed=5, draw=Draw()), plain)
    assert torch.equal(m.decode(codes, voice, seed=5, draw=[Draw()] * 3), plain)
    assert not m._sampler[1].last["draw"]                             # neutral records: no table was passed
    g1 = m.decode(codes, voice, seed=1, draw=Draw.greedy())
    g2 = m.decode(codes, voice, seed=2, draw=Draw.greedy())
    assert m._sampler[1].last["draw"] and torch.equal(g1, g2) and not torch.equal(g1, plain)
    m.draw = Draw.greedy()                                            # the model's default
    assert torch.equal(m.decode(codes, voice, seed=3), g1)
    assert torch.equal(m.decode(codes, voice, seed=5, draw=Draw()), plain)        # the argument wins
    m.draw = None
    with pytest.raises(S.L.AewError):
        m.decode(codes, voice, seed=5, draw=[Draw()] * 2)
    # decode_utterances: a record follows its utterance into the slot stream_groups assigns (two groups: 16 + 2)
    n_codes = [(7, 9, 10)[u % 3] for u in range(18)]
    utts = [torch.randint(0, K, (n,), generator=gen).to(DEV) for n in n_codes]
    voices = [(3 * u) % 40 for u in range(18)]
    recs = [RECORDS[(u + 3) % 8] for u in range(18)]
    out = m.decode_utterances(utts, voice=voices, seed=9, batch=3, draw=recs)
    eng, cg = m._utterance_engine("test", 3)
    lengths = [cg.L(n) for n in n_codes]
    groups = CD.stream_groups(lengths, 9)
    assert [len(mem) for _, mem in groups] == [16, 2] and lengths[groups[0][1][0]] > lengths[groups[1][1][0]] > 0
    assert len({lengths[u] for u in groups[0][1]}) > 1
    smp = m._engine_sampler(eng)
    rf, zero = smp.g.rf(), m.zero_amplitude_code()
    for g_seed, members in groups:
        cond, bias, got = m._conditioning_of(eng, cg, [utts[u] for u in members], [voices[u] for u in members], 16)
        forced = torch.full((16, cond.shape[1]), -1, dtype=torch.int32, device=DEV)
        for k, u in enumerate(members):
            forced[k, :min(lengths[u], rf + 1)] = zero
        n = len(members)
        if n < 16:
            cond[n:], bias[n:], forced[n:] = cond[0], bias[0], forced[0]
        table = draw_table([recs[u] for u in members] + [recs[members[0]]] * (16 - n), 16)
        wav, _ = smp.generate(cond, bias, forced, seed=g_seed, draw=table)
        for k, u in enumerate(members):
            assert torch.equal(out[u], wav[k, :lengths[u]].float()), u
    neutral_out = m.decode_utterances(utts, voice=voices, seed=9, batch=3, draw=[Draw()] * 18)
    assert all(torch.equal(a, b) for a, b in zip(neutral_out, m.decode_utterances(utts, voice=voices, seed=9, batch=3)))
    # convert: one window into 3 voices, one Draw per voice
    voice_to = torch.tensor([2, 11, 25], device=DEV)
    three = [Draw(0.8), Draw.greedy(), Draw(top_k=20)]
    c1 = m.convert(wav1, mel1, voice_to, seed=1, draw=three)
    c2 = m.convert(wav1, mel1, voice_to, seed=2, draw=three)
    assert c1.shape == (3, m.dec_in_len) and torch.equal(c1[1], c2[1]) and not torch.equal(c1[0], c2[0])
