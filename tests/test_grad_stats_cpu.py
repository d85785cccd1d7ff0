"""Gradient noise statistics without a GPU: the numpy restatement of AEW_OP_GRAD_WELFORD / AEW_OP_SEG_SELECT
(tests/grad_stats_emulator.py) against the fixture the reference's own grad_analysis.py produced
(tests/golden/grad_stats.npz), the order key the kernels call (aew_select_key) against the emulator's and torch.kthvalue,
the chunk table and scratch size against hand counts, every argument error of the two launchers, and the module surface
(argument names of the reference, the sharded data-parallel refusal)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L
from tests import grad_stats_emulator as E

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "grad_stats.npz"))
TAKING_PART = [n for n in GOLD["names"] if n != str(GOLD["no_grad"])]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------
# the emulator against the reference's recorded run
# ----------------------------------------------------------------------------------------------
def test_emulator_reproduces_the_reference_state_bit_for_bit_and_its_quantiles_as_numbers():
    n_batch, qs = int(GOLD["n_batch"]), list(GOLD["quantiles"])
    assert n_batch == 5 and qs == [0, 0.1, 0.25, 0.5, 0.75, 0.9, 1] and sorted(TAKING_PART) == ["a", "c", "d"]
    saw_nan = False
    for n in TAKING_PART:
        seq = GOLD["seq_" + n]
        mu = s = None
        for b in range(n_batch):                         # the reference's convention: the loop index is the count
            mu, s = E.welford(seq[b + 1], mu, s, b == 0, b)
            assert bits(mu).tobytes() == bits(GOLD["mu_" + n][b]).tobytes(), (n, b)
            assert bits(s).tobytes() == bits(GOLD["s_" + n][b]).tobytes(), (n, b)
        got = [E.kth(s, k, raw=False, denom=n_batch) for k in E.ranks(qs, s.size)]
        assert E.same_numbers(got, GOLD["quant_" + n]), (n, got, GOLD["quant_" + n])
        saw_nan |= bool(np.isnan(GOLD["quant_" + n]).any())
    assert saw_nan and (GOLD["s_c"][-1] < 0).any(), "the fixture holds the reference's own negative s / NaN quantile"


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F7FFFFF, 0x3F800001,
                    0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0xBF800000, 0x80800000,
                    0xC0400000, 0x40400000], np.uint32)


def test_select_key_of_the_library_is_the_emulators_on_the_special_values():
    lib = L.load()
    want = E.select_key(SPECIAL.view(np.float32))
    got = np.array([L.select_key(int(b)) for b in SPECIAL], np.uint32)
    assert got.tobytes() == want.tobytes()
    by = dict(zip(SPECIAL.tolist(), got.tolist()))
    assert by[0x80000000] == by[0] == 0 and by[0x00000001] == 1 and by[0x7F800000] == 0x7F800000
    assert all(by[b] == 0xFFFFFFFF for b in (0x80000001, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0xBF800000))
    assert by[0x3F7FFFFF] < by[0x3F800000] < by[0x3F800001] < by[0x7F7FFFFF] < by[0x7F800000]
    rs = np.random.RandomState(0)
    rnd = rs.randint(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    got = np.array([L.select_key(int(b)) for b in rnd], np.uint32)
    assert lib.aew_select_key(0, None) == L.E_ARG
    assert got.tobytes() == E.select_key(rnd.view(np.float32)).tobytes()


def test_emulator_selection_agrees_with_torch_kthvalue_after_the_references_sqrt():
    x = np.concatenate([SPECIAL.view(np.float32), np.float32([3, np.nan, 1, -0.0, 0.0, np.inf])])
    # (denom = 1: a NEGATIVE s whose quotient s / denom underflows to -0 - the negative denormal here, under denom = 4 - is
    #  -0 to the reference's sqrt and the NaN key to the op, whose key is that of s alone; include/aewavenet.h says so)
    with np.errstate(invalid="ignore"):
        ref = torch.from_numpy(x / np.float32(1)).sqrt()
    for k in range(1, x.size + 1):
        want = ref.kthvalue(k)[0].numpy()
        assert E.same_numbers([E.kth(x, k, raw=False, denom=1.0)], [want]), (k, want)
    pos = x[~(x < 0)]                                    # without the negatives any denominator agrees
    with np.errstate(invalid="ignore"):
        ref = torch.from_numpy(pos / np.float32(4)).sqrt()
    for k in range(1, pos.size + 1):
        assert E.same_numbers([E.kth(pos, k, raw=False, denom=4.0)], [ref.kthvalue(k)[0].numpy()]), k
    small = np.float32([3, np.nan, 1, -0.0, 0.0, np.inf])
    got = [E.kth(small, k) for k in range(1, 7)]
    assert E.same_numbers(got, np.float32([0, 0, 1, 3, np.inf, np.nan]))
    assert np.isnan(E.kth(small, 0)) and np.isnan(E.kth(small, 7)) and np.isnan(E.kth(small[:0], 1))


SIZES = [1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5, 70001, 0]


def test_chunk_table_ranks_and_scratch_size_against_hand_counts():
    offs, total = E.padded_offsets(SIZES)
    chunks, first = L.uw_chunks(offs, SIZES)
    want, wfirst = E.chunk_table(offs, SIZES)
    assert first == wfirst == [0, 1, 2, 3, 4, 5, 7, 11, 29, 29]
    assert [(chunks[i].off, chunks[i].len, chunks[i].tensor) for i in range(first[-1])] == want
    assert E.ranks([0, 0.1, 0.25, 0.5, 0.75, 0.9, 1], 4099) == [1, 411, 1025, 2050, 3075, 3689, 4099]
    assert E.ranks([0.5], 2) == [1] and E.ranks([0.5], 4) == [3] and E.ranks([0.5, 1], 1) == [1, 1]     # half to even
    from ae_wavenet_amd import grad_analysis as GA
    assert GA.ranks([0, 0.1, 0.5, 1], 70001) == E.ranks([0, 0.1, 0.5, 1], 70001) == [1, 7001, 35001, 70001]
    p, nbytes = L.SegSelect(), C.c_int64()
    for P, Q in ((1, 1), (9, 8), (196, 7)):
        p.n_tensors, p.Q = P, Q
        assert L.load().aew_seg_select_size(C.byref(p), C.byref(nbytes)) == 0
        assert nbytes.value == (P * Q * (256 + 2) * 4 + 15) // 16 * 16       # hist [P][Q][256], prefix and rank [P][Q]
    for P, Q in ((0, 1), (1, 0), (1, 9)):
        p.n_tensors, p.Q = P, Q
        assert L.load().aew_seg_select_size(C.byref(p), C.byref(nbytes)) == L.E_ARG
    assert L.load().aew_seg_select_size(None, C.byref(nbytes)) == L.E_ARG


def test_abi_version_and_mirrors():
    lib = L.load()
    assert lib.aew_abi_version() == 28                   # held: the additions are append-only, found through aew_sizeof
    assert lib.aew_sizeof(24) == -1 and C.sizeof(L.Op) == lib.aew_sizeof(0)
    assert lib.aew_sizeof(22) == C.sizeof(L.GradWelford) and lib.aew_sizeof(23) == C.sizeof(L.SegSelect)
    assert (L.OP_GRAD_WELFORD, L.OP_SEG_SELECT) == (32, 33) and L.SELECT_MAX_Q == 8
    assert L.OP_FIELD[L.OP_GRAD_WELFORD] == "gwel" and L.OP_FIELD[L.OP_SEG_SELECT] == "ssel"
    assert "aew_select_key" in L.EXPORTS and "aew_seg_select_size" in L.EXPORTS


# ----------------------------------------------------------------------------------------------
# argument errors: returned before any HIP call, so they are reachable without a device
# ----------------------------------------------------------------------------------------------
def run_rc(kind, field, **kw):
    op = L.Op()
    op.kind = kind
    p = getattr(op.u, field)
    for k, v in kw.items():
        setattr(p, k, v)
    fail = C.c_int(-1)
    return L.load().aew_run_plan(C.byref(op), 1, None, C.byref(fail))


OFFS, TOTAL = E.padded_offsets(SIZES[:4])
CHUNKS, FIRST = L.uw_chunks(OFFS, SIZES[:4])
G, MU, S, PART = 0x100000, 0x200000, 0x300000, 0x400000


def welford(**over):
    kw = dict(g=G, mu=MU, s=S, n=TOTAL, first=0, divisor=2.0)
    kw.update(over)
    return run_rc(L.OP_GRAD_WELFORD, "gwel", **kw)


def with_part(**over):
    kw = dict(part=PART, chunks=0x500000, chunks_host=C.addressof(CHUNKS), n_chunks=FIRST[-1])
    kw.update(over)
    return welford(**kw)


def test_welford_launcher_refuses_before_any_launch():
    assert welford(n=0) == 0 and welford(n=0, g=None, mu=None, s=None, first=1) == 0      # nothing to do: no launch either
    for over in (dict(n=-1), dict(g=None), dict(mu=None), dict(s=None), dict(first=2), dict(first=-1), dict(divisor=0.0),
                 dict(divisor=-1.0), dict(divisor=float("nan")), dict(mu=G), dict(s=G + 16), dict(s=MU + 4 * TOTAL - 16),
                 dict(mu=G - 4 * TOTAL + 16)):
        assert welford(**over) == L.E_ARG, over
    for over in (dict(g=G + 4), dict(mu=MU + 8), dict(s=S + 2)):
        assert welford(**over) == L.E_ALIGN, over
    assert welford(g=G + 4, divisor=0.0) == L.E_ARG                       # malformed comes before misaligned
    # with the chunk sums: the table must be there and cover [0, n) without a gap
    for over in (dict(chunks=None), dict(chunks_host=None), dict(n_chunks=0), dict(n_chunks=FIRST[-1] - 1), dict(n=TOTAL + 4)):
        assert with_part(**over) == L.E_ARG, over
    gap, _ = L.uw_chunks([0, 8, 12, 16], SIZES[:4])                       # a hole of four elements behind the first tensor
    assert with_part(chunks_host=C.addressof(gap)) == L.E_ARG
    assert with_part(part=PART + 8) == L.E_ALIGN


def select(**over):
    kw = dict(s=S, chunks=0x500000, n_chunks=FIRST[-1], n_tensors=4, Q=7, k=0x600000, out=0x700000, denom=5.0, raw=0,
              scratch=0x800000)
    kw.update(over)
    return run_rc(L.OP_SEG_SELECT, "ssel", **kw)


def test_select_launcher_refuses_before_any_launch():
    for over in (dict(Q=0), dict(Q=9), dict(n_tensors=0), dict(k=None), dict(out=None), dict(scratch=None), dict(s=None),
                 dict(chunks=None), dict(denom=0.0), dict(denom=-2.0), dict(denom=float("nan")), dict(raw=2), dict(n_chunks=-1)):
        assert select(**over) == L.E_ARG, over
    for over in (dict(s=S + 4), dict(scratch=0x800008), dict(chunks=0x500004), dict(k=0x600002), dict(out=0x700001)):
        assert select(**over) == L.E_ALIGN, over
    assert select(Q=9, s=S + 4) == L.E_ARG


# ----------------------------------------------------------------------------------------------
# the module surface
# ----------------------------------------------------------------------------------------------
def test_module_has_the_references_names_and_arguments():
    from ae_wavenet_amd import grad_analysis as GA
    assert list(inspect.signature(GA.grad_stats).parameters)[:4] == list(GOLD["args_grad_stats"])
    extra = list(inspect.signature(GA.grad_stats).parameters.values())[4:]
    assert [p.name for p in extra] == ["reference_counts"] and extra[0].kind is inspect.Parameter.KEYWORD_ONLY \
        and extra[0].default is True
    assert inspect.signature(GA.GradStats).parameters["reference_counts"].default is False
    assert "overwritten" in GA.grad_stats.__doc__ and "negative" in GA.grad_stats.__doc__


def test_add_under_the_sharded_schedule_raises_and_touches_nothing():
    from ae_wavenet_amd import autoencoder_model as ae, dp, grad_analysis as GA
    from tests.test_dp_gloo import _tiny
    model = ae.AutoEncoder(_tiny("vqvae-ema"), n_mel=5)
    d = dp.DataParallel.__new__(dp.DataParallel)         # (no process group: add() must refuse before it needs one)
    d.world, d.rank, d.force_collectives, d.group = 2, 0, False, None
    d.sharded = True
    model._dp = d
    gs = GA.GradStats(model)
    with pytest.raises(L.AewError, match="sharded data-parallel schedule: each rank holds the reduced gradient of its own shards only"):
        gs.add()
    assert gs.count == 0 and gs.mu is None and gs.s is None
    with pytest.raises(L.AewError):
        gs.sigma_quantiles([0.5])
