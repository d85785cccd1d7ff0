"""The device-resident corpus without a GPU: the numpy restatement of AEW_OP_WINDOW_GATHER (tests/corpus_emulator.py)
against the reference's recorded run (tests/golden/corpus_order.json, written by tests/golden/make_corpus_golden.py);
aew_corpus_locate - compiled from the helper the kernel calls - against the emulator; the launcher's refusals, which
come before any launch and so need no device; the ABI mirror; the host side of ae_wavenet_amd/corpus.py (tables,
restricted unpickler, resume state)."""
import ctypes as C
import json
import os
import pickle
import sys
import types
from collections import namedtuple

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, corpus as CP
from tests import corpus_emulator as E
from tests.conftest import GOLDEN

RUNS = json.load(open(os.path.join(GOLDEN, "corpus_order.json")))
CASES = [(r["num_replicas"], r["rank"]) for r in RUNS["runs"]]


def recorded(R, rank):
    return next(r for r in RUNS["runs"] if (r["num_replicas"], r["rank"]) == (R, rank))


def test_golden_file_is_the_issue_s_corpus():
    assert CASES == [(1, 0), (3, 0), (3, 1), (3, 2)]
    assert (tuple(RUNS["lengths"]), RUNS["slice_size"], RUNS["n_win_batch"], RUNS["batch_size"]) == (E.LENGTHS, 40, 7, 4)
    assert all(len(r["batches"]) == 12 and r["n_slices"] == 29 for r in RUNS["runs"])


@pytest.mark.parametrize("R,rank", CASES)
def test_emulator_reproduces_the_reference_run(R, rank):
    snd, samples = E.golden_corpus()
    em = E.Emulator(snd, samples, E.SLICE, E.STRIDE, R, rank)
    assert (em.N, em.n_order) == (29, len(range(rank, 29, R)))
    straddles = 0
    for rec in recorded(R, rank)["batches"]:
        t0 = em.t
        got = em.batch(4)
        assert got["starts"] == [x[0] for x in rec]
        assert got["voice"].tolist() == [x[1] for x in rec]
        assert got["position"].tolist() == rec[-1][2:]                   # the LAST item's (epoch, step)
        for b, x in enumerate(rec):                                      # and every item's, as a batch of one ending there
            assert list(E.locate(t0 + b, 0, 1, em.N, em.n_order, R)[2:]) == x[2:]
        for b in range(4):
            assert np.array_equal(got["wav"][b], snd[rec[b][0]:rec[b][0] + 40].astype(np.float32))
        straddles += t0 // em.n_order != (t0 + 3) // em.n_order
    assert straddles >= 1                                                # a batch that crosses sampler epochs is in the run


def c_locate(t0, b, B, N, n_order, R, rank):
    e, p, pe, ps = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    rc = L.load().aew_corpus_locate(t0, b, B, N, n_order, R, rank, C.byref(e), C.byref(p), C.byref(pe), C.byref(ps))
    assert rc == 0, rc
    return e.value, p.value, pe.value, ps.value


@pytest.mark.parametrize("R,rank", CASES)
def test_locate_agrees_with_the_emulator_on_the_golden_runs(R, rank):
    n_order = len(range(rank, 29, R))
    for k in range(12):
        for b in range(4):
            assert c_locate(4 * k, b, 4, 29, n_order, R, rank) == E.locate(4 * k, b, 4, 29, n_order, R)


@pytest.mark.parametrize("t0,B,N,n_order,R,rank", [
    ((1 << 33) - 3, 8, 29, 10, 3, 1), ((1 << 33) + 12345, 8, 4_000_003, 500_001, 8, 0),      # t0 near 2^33
    (0, 1, 29, 29, 1, 0), (57, 1, 29, 9, 3, 2), (1 << 33, 1, 29, 10, 3, 0),                   # B = 1
    (0, 9, 29, 9, 3, 2), (9 * 1000 + 4, 9, 29, 9, 3, 2), (29 * 7, 29, 29, 29, 1, 0)])        # n_order == B
def test_locate_edge_cases(t0, B, N, n_order, R, rank):
    for b in sorted({0, B // 2, B - 1}):
        assert c_locate(t0, b, B, N, n_order, R, rank) == E.locate(t0, b, B, N, n_order, R)


def test_locate_refuses_nonsense():
    lib, z, z64 = L.load(), C.c_int(), C.c_int64()
    out = (C.byref(z), C.byref(z), C.byref(z64), C.byref(z64))
    assert lib.aew_corpus_locate(0, 4, 4, 29, 10, 3, 0, *out) == L.E_ARG           # b outside the batch
    assert lib.aew_corpus_locate(0, 0, 4, 29, 10, 3, 3, *out) == L.E_ARG           # rank >= R
    assert lib.aew_corpus_locate(0, 0, 4, 29, 0, 3, 0, *out) == L.E_ARG            # empty order
    assert lib.aew_corpus_locate(1 << 40, 0, 1, 1, 1, 1, 0, *out) == L.E_ARG       # epoch does not fit an int
    assert lib.aew_corpus_locate(0, 0, 4, 29, 10, 3, 0, None, C.byref(z), C.byref(z64), C.byref(z64)) == L.E_ARG


# ----------------------------------------------------------------------------------------------
# the launcher's checks: aew_run_plan reaches them without a device and returns before any launch
# ----------------------------------------------------------------------------------------------
def descriptor(**over):
    """A descriptor that passes every check (made-up addresses: it is never launched here), fields overridden."""
    g = L.WindowGather()
    g.snd, g.n_snd, g.snd_bytes, g.B = 0x10000, 417, 1, 4
    g.starts, g.voices, g.N = 0x20000, 0x30000, 29
    g.order, g.n_order, g.num_replicas, g.rank, g.advance, g.counter = 0x40000, 9, 3, 2, 1, 0x50000
    g.slice_size, g.wav_pitch = 40, 40
    g.wav, g.voice, g.index, g.position = 0x60000, 0x70000, 0x80000, 0x90000
    for k, v in over.items():
        assert hasattr(g, k)
        setattr(g, k, v)
    return g


def run_plan_rc(g):
    op = L.Op()
    op.kind = L.OP_WINDOW_GATHER
    op.u.wgat = g
    ops, fail = (L.Op * 1)(op), C.c_int(-1)
    rc = L.load().aew_run_plan(C.cast(ops, C.c_void_p), 1, None, C.byref(fail))
    assert fail.value == 0
    return rc


@pytest.mark.parametrize("over,want", [
    (dict(n_order=3), L.E_ARG),                          # n_order < B
    (dict(slice_size=0), L.E_ARG), (dict(slice_size=-5), L.E_ARG),
    (dict(snd_bytes=3), L.E_ARG), (dict(snd_bytes=0), L.E_ARG), (dict(snd_bytes=8), L.E_ARG),
    (dict(rank=3), L.E_ARG), (dict(rank=-1), L.E_ARG),   # rank outside [0, R)
    (dict(n_order=10), L.E_ARG),                         # not len(range(rank, N, R)): an index could leave the table
    (dict(wav_pitch=42), L.E_ARG), (dict(wav_pitch=36), L.E_ARG), (dict(n_snd=39), L.E_ARG),
    (dict(B=0), L.E_ARG), (dict(counter=0), L.E_ARG), (dict(position=0), L.E_ARG),
    (dict(snd=0x10001), L.E_ALIGN),                      # the corpus at base + 1
    (dict(wav=0x60004), L.E_ALIGN), (dict(starts=0x20004), L.E_ALIGN), (dict(order=0x40002), L.E_ALIGN),
    (dict(snd_bytes=3, snd=0x10001), L.E_ARG)])          # malformed comes before misaligned
def test_launcher_refuses_before_any_launch(over, want):
    assert run_plan_rc(descriptor(**over)) == want


def test_abi_version_and_mirror():
    lib = L.load()
    assert lib.aew_abi_version() == 28
    assert lib.aew_sizeof(21) == C.sizeof(L.WindowGather)
    assert L.OP_WINDOW_GATHER == 31 and L.OP_FIELD[L.OP_WINDOW_GATHER] == "wgat"
    assert "aew_corpus_locate" in L.EXPORTS


# ----------------------------------------------------------------------------------------------
# corpus.py on the host: tables, the restricted unpickler, resume state
# ----------------------------------------------------------------------------------------------
def test_tables_follow_the_reference():
    snd, samples = E.golden_corpus()
    c = CP.DeviceCorpus(snd, samples, 40, 7, None, num_replicas=3, rank=2)
    assert (len(c), c.n_order, c.num_speakers()) == (29, 9, 3)
    rec = recorded(3, 2)
    rows = set(zip(c.starts_host.tolist(), c.voices_host.tolist()))
    assert all((x[0], x[1]) in rows for bt in rec["batches"] for x in bt)
    assert list(zip(c.starts_host.tolist(), c.voices_host.tolist())) == E.table(samples, 40, 7)
    for e in range(3):                                    # the rows it would upload are the emulator's
        assert c.cursor.row(e).tolist() == E.order_row(e, 9, 3, 2)
    assert CP.DeviceCorpus(snd, samples, 40, 7, None, 3, 2, start_epoch=5).cursor.row(1).tolist() == E.order_row(6, 9, 3, 2)
    with pytest.raises(L.AewError):                       # no CPU path
        c.gather_op(4, torch.zeros(4, 40), torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                    torch.zeros(2, dtype=torch.int64))
    with pytest.raises(L.AewError):
        CP.DeviceBatches(c, 4)
    with pytest.raises(ValueError):
        CP.DeviceCorpus(snd, samples, 40, 7, None, num_replicas=3, rank=3)
    with pytest.raises(TypeError):
        CP.DeviceCorpus(snd.astype(np.float32), samples, 40, 7, None)
    with pytest.raises(ValueError):
        CP.DeviceCorpus(snd[:400], samples, 40, 7, None)
    import ae_wavenet_amd
    assert ae_wavenet_amd.DeviceCorpus is CP.DeviceCorpus and ae_wavenet_amd.DeviceBatches is CP.DeviceBatches


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_from_dat_reads_the_reference_s_pickle(tmp_path, monkeypatch, dtype):
    snd, samples = E.golden_corpus()
    snd = (snd.astype(np.int64) * (1 if dtype == np.uint8 else 100) - (0 if dtype == np.uint8 else 9000)).astype(dtype)
    mod = types.ModuleType("data")                        # a throwaway `data` module, for the dump only
    mod.SpokenSample = namedtuple("SpokenSample", CP.SpokenSample._fields, module="data")
    monkeypatch.setitem(sys.modules, "data", mod)
    recs = [mod.SpokenSample(v, b, e, f"utt{i}.wav") for i, (v, b, e) in enumerate(samples)]
    path = tmp_path / "corpus.dat"
    with open(path, "wb") as fh:
        pickle.dump({"samples": recs, "snd_dtype": dtype, "snd_data": snd}, fh)
    monkeypatch.delitem(sys.modules, "data")
    got = CP.DeviceCorpus.from_dat(str(path), 40, 7, None, num_replicas=3, rank=1)
    want = CP.DeviceCorpus.from_arrays(snd, samples, 40, 7, None, num_replicas=3, rank=1)
    assert "data" not in sys.modules                      # read without the module that wrote it
    assert got.snd_host.dtype == dtype and np.array_equal(got.snd_host, want.snd_host)
    assert np.array_equal(got.starts_host, want.starts_host) and np.array_equal(got.voices_host, want.voices_host)
    assert (got.N, got.n_order, got.snd_bytes, got.num_speakers()) == (29, 10, np.dtype(dtype).itemsize, 3)
    assert all(type(s) is CP.SpokenSample for s in got.samples) and got.samples[4].file_path == "utt4.wav"


def test_from_dat_refuses_any_other_global(tmp_path):
    snd, _ = E.golden_corpus()
    for i, payload in enumerate(({"samples": [], "snd_dtype": np.uint8, "snd_data": snd, "extra": os.getcwd},
                                 {"samples": [types.SimpleNamespace(voice_index=0)], "snd_dtype": np.uint8, "snd_data": snd},
                                 {"samples": [], "snd_dtype": np.float64, "snd_data": snd})):
        path = tmp_path / f"bad{i}.dat"
        with open(path, "wb") as fh:
            pickle.dump(payload, fh)
        with pytest.raises(pickle.UnpicklingError):
            CP.DeviceCorpus.from_dat(str(path), 40, 7, None)


def test_state_round_trip_on_the_mirror():
    snd, samples = E.golden_corpus()
    a = CP.DeviceCorpus(snd, samples, 40, 7, None, num_replicas=3, rank=2)
    a.cursor.seek(23)
    state = a.state_dict()
    assert state == {"items": 23, "num_replicas": 3, "rank": 2, "n_slices": 29, "start_epoch": 0}
    b = CP.DeviceCorpus(snd, samples, 40, 7, None, num_replicas=3, rank=2)
    b.load_state_dict(state)
    assert b.state_dict() == state and b.cursor.position() == (2, 9) == tuple(E.locate(19, 0, 4, 29, 9, 3)[2:])
    for other in (dict(num_replicas=3, rank=1), dict(num_replicas=1, rank=0)):                 # changed rank / R
        with pytest.raises(ValueError):
            CP.DeviceCorpus(snd, samples, 40, 7, None, **other).load_state_dict(state)
    with pytest.raises(ValueError):                                                            # changed N
        CP.DeviceCorpus(snd, samples, 40, 5, None, num_replicas=3, rank=2).load_state_dict(state)
    with pytest.raises(ValueError):
        b.load_state_dict(dict(state, items=-1))
