"""VQ codes as an interface, without a GPU: the appended ABI records, the decode plan of a TrainEngine built on 'cpu'
(the lookup in front of the unchanged conditioning plan; where the encode and decode plans write), the refusal of
models without discrete codes, and the numpy restatement of the run-length collapse against itertools.groupby."""
import ctypes as C
import importlib.util
import itertools
import json
import os

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, autoencoder_model as ae, codes as CD, config, mfcc_inverter as mi, model as M
from tests import codes_emulator as CE
from tests.plan_emulator import Emu
from tests.test_evaluate_cpu import OUTPUTS, protected

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("plan_gen_codes", os.path.join(HERE, "data", "plan_gen.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

RUN_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2500)       # the lengths tests/test_codes_gpu.py runs on the device
OUTPUTS = dict(OUTPUTS)
OUTPUTS[L.OP_CODE_LOOKUP] = lambda e, p: [p.zq, p.bad]


def test_appended_records_and_unchanged_abi():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert lib.aew_sizeof(27) == C.sizeof(L.CodeLookup) and lib.aew_sizeof(28) == C.sizeof(L.CodeRuns)
    assert lib.aew_sizeof(24) == -1 and lib.aew_sizeof(26) == -1
    # the two records fit the union: sizeof(aew_op_t) is what the GEMM descriptor makes it, as before
    assert lib.aew_sizeof(0) == C.sizeof(L.Op) == 16 + C.sizeof(L.GemmNT)
    assert max(C.sizeof(L.CodeLookup), C.sizeof(L.CodeRuns)) < C.sizeof(L.GemmNT)
    assert (L.OP_CODE_LOOKUP, L.OP_CODE_RUNS) == (L.OP_ACCUM + 1, L.OP_ACCUM + 2)


def _training_state(eng):
    """{name: whole workspace buffer} of everything the encode and decode plans must leave alone."""
    out = protected(eng)                                  # loss_buf, met_buf, diag, moments, params, grads, the EMA buffers
    out.pop("n_sum_diag", None)                           # (scratch of the forward: fwd_a rewrites it before fwd_b reads it)
    if eng.bn_type == "vqvae-ema":
        for n in ("z_sum", "n_sum"):
            t = getattr(eng, n)
            out[n] = eng.ws.get(eng.ws.resolve(t.data_ptr())[0])
    return out


@pytest.mark.parametrize("bn", ["vqvae", "vqvae-ema"])
def test_decode_plan_is_the_lookup_in_front_of_the_conditioning_plan(bn):
    name = f"default.{bn}"
    with open(gen.TABLE) as f:
        want = json.load(f)["configs"][name]
    eng = gen.build(gen.configs()[name])
    parent = gen.allocations(eng)
    assert gen.digest(parent) == want["alloc"]            # an engine that has not decoded: the parent's allocations
    assert eng._decode_plan is None and eng.codes_bad is None and "codes.bad" not in eng.ws.bufs
    eng._cond_plans()                                      # the encode half allocates nothing
    assert gen.allocations(eng) == parent
    dp = eng.decode_plan()
    assert eng.decode_plan() is dp                         # built once
    assert [a[0] for a in gen.allocations(eng)[len(parent):]] == ["codes.bad"] and gen.allocations(eng)[:len(parent)] == parent
    # [lookup] + the ops of _cond_plan, the same records - all but the codebook diagnostics, which sit in that prefix of
    # fwd_b and write `diag` (from encoder outputs a decode never computed)
    cp = eng._cond_plan
    drop = [i for i, l in enumerate(cp.labels) if l in M.TrainEngine.DECODE_DROP]
    assert [cp.ops[i].kind for i in drop] == [L.OP_VQ_DIAG] and cp.ops[drop[0]].u.diag.out == eng.diag.data_ptr()
    kept = [i for i in range(len(cp.ops)) if i not in drop]
    assert dp.labels == ["code.lookup"] + [cp.labels[i] for i in kept] and len(kept) > 3
    assert dp.ops[0].kind == L.OP_CODE_LOOKUP and dp.ops[0].lane == 0
    for a, i in zip(dp.ops[1:], kept):                     # the same records
        assert a is cp.ops[i]
    for a, i in zip(dp.array()[1:], kept):
        assert bytes(a) == bytes(cp.array()[i])
    lk, vq = dp.ops[0].u.clk, eng.fwd_a.ops[eng.fwd_a.labels.index("vq.nearest")].u.vqn
    assert (lk.ind, lk.emb, lk.zq, lk.Q, lk.K, lk.d, lk.d_pitch) == (vq.ind, vq.emb, vq.zq, vq.Q, vq.K, vq.d, vq.d_pitch)
    bad = eng.codes_bad
    assert lk.bad == bad.data_ptr()
    for n, t in eng.ws.bufs.items():                       # a word of its own: inside no other buffer
        assert n == "codes.bad" or not (t.data_ptr() <= lk.bad < t.data_ptr() + t.numel() * t.element_size())
    # no op of the encode and decode plans writes through an address inside a training-state buffer
    assert "vq.stats" not in eng._cond_plan_a.labels and "vq.ema" not in dp.labels
    emu = Emu(eng.ws)
    ranges = {k: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for k, t in _training_state(eng).items()}
    assert {"loss_buf", "met_buf", "diag", "params", "grads", "adam_m", "adam_v"} <= set(ranges)
    assert bn != "vqvae-ema" or {"emb", "ema_numer", "ema_denom", "ind_hist", "z_sum", "n_sum"} <= set(ranges)
    for pl in (eng._cond_plan_a, dp):
        for op, lab in zip(pl.array(), pl.labels):
            assert op.kind in OUTPUTS, (lab, op.kind)
            for ptr in OUTPUTS[op.kind](emu, getattr(op.u, L.OP_FIELD[op.kind])):
                for k, (lo, hi) in ranges.items():
                    assert not (ptr and lo <= ptr < hi), (lab, k)


def test_codes_to_conditioning_bumps_the_activation_epoch_and_checks_its_argument():
    eng = gen.build(gen.configs()["default.vqvae-ema"])
    ran = []
    eng._run = lambda plan, timing=False: ran.append(plan.name)
    e0 = eng.act_epoch
    codes = torch.arange(eng.Q).view(eng.B, -1) % eng.K
    eng.bn.ind.zero_()
    cond, bias = eng.codes_to_conditioning(codes)
    assert ran == ["codes_to_conditioning"] and eng.act_epoch == e0 + 1
    assert torch.equal(eng.ind[:eng.Q], codes.reshape(-1)) and int(eng.codes_bad[0]) == 0
    assert cond.data_ptr() == eng.dec.cond.tensor().data_ptr() and bias.shape[0] == eng.B
    eng.encode_codes()
    assert ran[-1] == "conditioning_a" and eng.act_epoch == e0 + 2
    with pytest.raises(L.AewError):
        eng.codes_to_conditioning(codes[:, :-1])
    with pytest.raises(L.AewError):
        eng.codes_to_conditioning(codes.int())
    other = gen.build(gen.configs()["default.vae"])
    with pytest.raises(L.AewError, match="vae"):
        other.codes_to_conditioning(codes)
    with pytest.raises(L.AewError, match="vae"):
        other.encode_codes()


def _small(kind):
    return config.make_hps(kind, n_res=8, n_dil=8, n_skp=8, n_post=8, n_lc_out=8, n_global_embed=2, n_speakers=3, n_blocks=1,
                           n_block_layers=2, n_win_batch=5, **({} if kind == "mi" else dict(enc_n_out=8, bn_n_out=4)))


@pytest.mark.parametrize("kind", ["vae", "ae", "mi"])
def test_models_without_codes_refuse_by_name(kind):
    m = mi.MfccInverter(_small(kind)) if kind == "mi" else ae.AutoEncoder(_small(kind), n_mel=5)
    name = "none" if kind == "mi" else kind
    codes, voice = torch.zeros(1, m.embed_len, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    for call in (lambda: m.encode(torch.zeros(1, 5, 8)), lambda: m.decode(codes, voice),
                 lambda: m.convert(torch.zeros(1, 8), torch.zeros(1, 5, 8), voice)):
        with pytest.raises(L.AewError, match=f"'{name}'"):
            call()


def test_zero_amplitude_encodes_to_the_middle_value():
    assert int(CD.mu_encode(torch.zeros(1), 256)[0]) == 128
    q = CD.mu_encode(torch.tensor([-1.0, -0.5, 0.0, 0.25, 1.0]), 256)
    assert q.tolist() == sorted(q.tolist()) and q[0] == 0 and q[-1] == 255
    m = ae.AutoEncoder(_small("vqvae"), n_mel=5)
    assert m.zero_amplitude_code() == 128


def _groupby(row):
    runs = [(k, len(list(g))) for k, g in itertools.groupby(row.tolist())]
    return [k for k, _ in runs], [n for _, n in runs]


@pytest.mark.parametrize("N", RUN_LENGTHS)
def test_emulator_runs_against_groupby(N):
    rows = CE.boundary_rows(N)
    units, lengths, n_runs = CE.code_runs(rows)
    assert units.dtype == np.int64 and lengths.dtype == np.int32 and n_runs.dtype == np.int32
    for b in range(rows.shape[0]):
        u, ln = _groupby(rows[b])
        n = len(u)
        assert n_runs[b] == n and units[b, :n].tolist() == u and lengths[b, :n].tolist() == ln
        assert (units[b, n:] == -1).all() and (lengths[b, n:] == 0).all() and lengths[b].sum() == N
    assert n_runs[2] == 1 and n_runs[3] == N
    if N > 64:                                             # the seams the rows are built for
        starts0 = np.flatnonzero(np.diff(rows[0])) + 1
        assert not set(starts0) & set(range(0, N, 64)) and len(starts0) >= (N - 4) // 64
        assert set(range(64, N, 64)) <= set(np.flatnonzero(np.diff(rows[1])) + 1)


def test_emulator_lookup_is_a_row_gather():
    rs = np.random.RandomState(0)
    emb = rs.randn(11, 6).astype(np.float32)
    ind = np.array([3, -1, 10, 11, 0], np.int64)
    zq, bad = CE.lookup(emb, ind, d_pitch=8)
    assert bad == 2 and not zq[[1, 3]].any() and not zq[:, 6:].any()
    assert zq[[0, 2, 4], :6].tobytes() == emb[[3, 10, 0]].tobytes()
