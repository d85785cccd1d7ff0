"""AEW_OP_WINDOW_GATHER and ae_wavenet_amd/corpus.py on the GPU, bit for bit against tests/corpus_emulator.py (which
tests/test_corpus_cpu.py holds to the reference's recorded run): the golden corpus through DeviceBatches; every source
alignment, the slice that ends on the corpus' last element, sizes around the 16-byte piece and one of several blocks per
row, for the three corpus dtypes, with guard bands around the output; the op in a captured graph (the DEVICE counter
drives the sequence); advance = 0; resume across a sampler epoch; the held-out pass; and one end-to-end training run."""
import ctypes as C

import numpy as np
import pytest
import torch

from ae_wavenet_amd import _lib as L, corpus as CP
from ae_wavenet_amd.plan import Plan
from tests import corpus_emulator as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def golden(R=1, rank=0, **kw):
    snd, samples = E.golden_corpus()
    return CP.DeviceCorpus(snd, samples, E.SLICE, E.STRIDE, DEV, num_replicas=R, rank=rank, **kw), \
        E.Emulator(snd, samples, E.SLICE, E.STRIDE, R, rank, **kw)


def same(got, want, index=None):
    wav, mel, voice, jit, position = got
    assert wav.dtype == torch.float32 and voice.dtype == torch.int64 and position.dtype == torch.int64
    assert np.array_equal(wav.cpu().numpy(), want["wav"])
    assert np.array_equal(voice.cpu().numpy(), want["voice"])
    assert np.array_equal(position.cpu().numpy(), want["position"])
    if index is not None:
        assert index.dtype == torch.int32 and np.array_equal(index.cpu().numpy(), want["index"])


@pytest.mark.parametrize("R,rank,prefetch", [(1, 0, 0), (3, 2, 0), (1, 0, 2), (3, 2, 1)])
def test_golden_corpus_through_device_batches(R, rank, prefetch):
    """prefetch > 0: the same batches, produced ahead on the iterator's own stream; position, index and the corpus'
    state speak of the batches handed out, the device counter of the batches issued."""
    corpus, em = golden(R, rank)
    it = CP.DeviceBatches(corpus, 4, prefetch=prefetch)
    assert it.position == (0, 0)
    for _ in range(12):
        got = next(it)
        want = em.batch(4)
        same(got, want, it.index)
        assert got[1] is None and got[3] is None
        assert it.position == tuple(want["position"].tolist()) == tuple(got[4].tolist())     # host mirror == device
    assert corpus.state_dict()["items"] == 48 == int(corpus.cursor.counter.item()) - 4 * prefetch


# ----------------------------------------------------------------------------------------------
# alignment and bounds: the op called directly on a hand-built table
# ----------------------------------------------------------------------------------------------
N_SND, GUARD, PATTERN = 4099 + 37, 64, -777.0


def source(dtype):
    rs = np.random.RandomState(7)
    if dtype == np.uint8:
        return rs.randint(0, 256, N_SND).astype(np.uint8)
    info = np.iinfo(dtype)
    snd = rs.randint(info.min, info.max, N_SND, dtype=np.int64).astype(dtype)
    snd[:4] = (info.min, info.max, -1, 0)
    return snd


@pytest.fixture(scope="module", params=[np.uint8, np.int16, np.int32], ids=["uint8", "int16", "int32"])
def resident(request):
    """(host corpus, device copy sized to the contract exactly: the elements + 16 bytes of slack, rounded up to 16)."""
    snd = source(request.param)
    raw = snd.view(np.uint8)
    dev = torch.zeros(-(-(raw.size + 16) // 16) * 16, dtype=torch.uint8, device=DEV)
    dev[:raw.size].copy_(torch.from_numpy(raw))
    assert dev.data_ptr() % 16 == 0
    return snd, dev


@pytest.mark.parametrize("n", [1, 15, 16, 17, 40, 4099])
def test_every_alignment_and_the_corpus_end(resident, n):
    snd, dev = resident
    B = 2
    starts = [16 + r for r in range(16)] + [N_SND - n, 0]            # every residue mod 16, the last element, the first
    N = len(starts)
    pitch = -(-n // 4) * 4
    d_starts = torch.tensor(starts, dtype=torch.int64, device=DEV)
    d_voices = torch.arange(100, 100 + N, dtype=torch.int32, device=DEV)
    order = torch.arange(N, dtype=torch.int32, device=DEV).repeat(2, 1).contiguous()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    n_launch = N // B
    buf = torch.full((GUARD + n_launch * B * pitch + GUARD,), PATTERN, dtype=torch.float32, device=DEV)
    voice = torch.full((N,), -5, dtype=torch.int64, device=DEV)
    index = torch.full((N,), -5, dtype=torch.int32, device=DEV)
    position = torch.zeros(n_launch, 2, dtype=torch.int64, device=DEV)
    assert (buf.data_ptr() + 4 * GUARD) % 16 == 0
    ops = (L.Op * n_launch)()
    for k in range(n_launch):
        g = L.WindowGather()
        g.snd, g.n_snd, g.snd_bytes, g.B = dev.data_ptr(), N_SND, snd.dtype.itemsize, B
        g.starts, g.voices, g.N = d_starts.data_ptr(), d_voices.data_ptr(), N
        g.order, g.n_order, g.num_replicas, g.rank, g.advance = order.data_ptr(), N, 1, 0, 1
        g.counter, g.slice_size, g.wav_pitch = counter.data_ptr(), n, pitch
        g.wav = buf.data_ptr() + 4 * (GUARD + k * B * pitch)
        g.voice, g.index = voice.data_ptr() + 8 * k * B, index.data_ptr() + 4 * k * B
        g.position = position.data_ptr() + 16 * k
        ops[k].kind = L.OP_WINDOW_GATHER
        ops[k].u.wgat = g
    fail = C.c_int(-1)
    st = torch.cuda.current_stream().cuda_stream
    L.check(L.load().aew_run_plan(C.cast(ops, C.c_void_p), n_launch, C.c_void_p(st), C.byref(fail)), "gather", fail.value)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:GUARD] == PATTERN).all()) and bool((got[-GUARD:] == PATTERN).all()), "guard band written"
    rows = got[GUARD:-GUARD].view(N, pitch)
    assert bool((rows[:, n:] == PATTERN).all()), "pad columns written"
    host = torch.from_numpy(snd)
    for i, s in enumerate(starts):
        assert torch.equal(rows[i, :n], host[s:s + n].float()), (i, s)
    assert voice.tolist() == list(range(100, 100 + N)) and index.tolist() == list(range(N))
    assert int(counter.item()) == N
    assert position.tolist() == [[(B * (k + 1)) // N, (B * (k + 1)) % N] for k in range(n_launch)]


# ----------------------------------------------------------------------------------------------
# the device counter drives the sequence
# ----------------------------------------------------------------------------------------------
def graph_outputs(corpus, advance, replays):
    B, n = 4, corpus.slice_size
    wav = torch.zeros(B, n, dtype=torch.float32, device=DEV)
    voice = torch.zeros(B, dtype=torch.int64, device=DEV)
    index = torch.zeros(B, dtype=torch.int32, device=DEV)
    position = torch.zeros(2, dtype=torch.int64, device=DEV)
    plan = Plan("corpus")
    plan.add(L.OP_WINDOW_GATHER, corpus.gather_op(B, wav, voice, index, position, advance=advance).u.wgat, "gather")
    st = torch.cuda.current_stream().cuda_stream
    out = []
    try:
        for _ in range(replays):
            if advance:
                corpus.note_batches(1)
            plan.run_graph(st)
            out.append((wav.clone(), None, voice.clone(), None, position.clone(), index.clone()))
        torch.cuda.synchronize()
    finally:
        plan.invalidate_graph()
    return out


def test_captured_graph_yields_consecutive_batches():
    corpus, em = golden()
    for got in graph_outputs(corpus, 1, 3):                          # ONE captured record, three replays
        same(got[:5], em.batch(4), got[5])
    assert int(corpus.cursor.counter.item()) == 12 == corpus.state_dict()["items"]


def test_advance_zero_repeats_the_batch():
    corpus, em = golden(3, 2)
    want = em.batch(4, advance=False)
    for got in graph_outputs(corpus, 0, 2):
        same(got[:5], want, got[5])
    assert int(corpus.cursor.counter.item()) == 0


@pytest.mark.parametrize("prefetch", [0, 2])
def test_resume_reproduces_the_uninterrupted_run(prefetch):
    whole, em = golden()
    it = CP.DeviceBatches(whole, 4)
    ref = [next(it) + (it.index,) for _ in range(9)]                 # batches 1..9; the 8th (items 28..31) crosses N = 29
    cut, _ = golden()
    it = CP.DeviceBatches(cut, 4, prefetch=prefetch)                 # (batches produced ahead are not part of the state)
    for _ in range(5):
        next(it)
    state = cut.state_dict()
    assert state["items"] == 20
    fresh, _ = golden()
    fresh.load_state_dict(state)
    it = CP.DeviceBatches(fresh, 4, prefetch=prefetch)
    for k in range(5, 9):                                            # batches 6..9
        got = next(it)
        for a, b in zip(got + (it.index,), ref[k]):
            assert (a is None and b is None) or torch.equal(a, b)
    for k in range(9):                                               # and the uninterrupted run is the emulator's
        same(ref[k][:5], em.batch(4), ref[k][5])
    assert (5 * 4) // 29 != (9 * 4 - 1) // 29


def test_held_out_pass_in_table_order():
    corpus, _ = golden()
    snd, samples = E.golden_corpus()
    em = E.Emulator(snd, samples, E.SLICE, E.STRIDE, shuffle=False)
    it = CP.DeviceBatches(corpus, 4, shuffle=False)
    sizes, rows = [], []
    for got in it:
        B = got[0].shape[0]
        same(got, em.batch(B), it.index)
        sizes.append(B)
        rows += it.index.tolist()
    assert sizes == [4] * 7 + [1] and rows == list(range(29))
    with pytest.raises(StopIteration):
        next(it)
    assert corpus.state_dict()["items"] == 0                         # the training order has not moved
    it.reset()
    assert next(it)[0].shape[0] == 4
    ahead = CP.DeviceBatches(corpus, 4, shuffle=False, prefetch=3)   # produced ahead: the same pass, the same end
    assert [b[0].shape[0] for b in ahead] == sizes
    ahead.reset()
    next(ahead)
    ahead.reset()                                                    # moved while batches are in flight: they are dropped
    assert ahead.position == (0, 0)
    next(ahead)
    assert ahead.index.tolist() == [0, 1, 2, 3] and ahead.position == (0, 4)


@pytest.mark.parametrize("prefetch", [0, 1])
def test_end_to_end_training_steps(prefetch):
    """Plumbing only: a corpus of random bytes -> DeviceBatches(mfcc, jitter) -> model.run -> backward -> FusedAdam, twice,
    at the smallest model tests/test_surface_gpu.py runs."""
    from ae_wavenet_amd import optim
    from ae_wavenet_amd.jitter import DeviceJitter
    from ae_wavenet_amd.mfcc import DeviceMfcc
    from tests.test_surface_gpu import _tiny
    hps, m = _tiny()
    n = m.geom.enc_in_len
    rs = np.random.RandomState(3)
    lengths = (n + 300, n + 1, n + 97 * 4 + 5)
    snd = rs.randint(0, 256, sum(lengths)).astype(np.uint8)
    samples, at = [], 0
    for i, ln in enumerate(lengths):
        samples.append((i % 5, at, at + ln))
        at += ln
    corpus = CP.DeviceCorpus(snd, samples, n, hps.n_win_batch, DEV)
    em = E.Emulator(snd, samples, n, hps.n_win_batch)
    assert len(corpus) == em.N == 4 + 1 + 5
    opt = optim.FusedAdam(m, lr=1e-4)
    it = CP.DeviceBatches(corpus, 2, mfcc=DeviceMfcc(DEV), jitter=DeviceJitter(0.12, seed=5), prefetch=prefetch)
    for _ in range(2):
        wav, mel, voice, jitter, position = next(it)
        assert mel.shape == (2, 39, m.geom.mel_len) and jitter.shape == (2, m.geom.mel_len)
        opt.zero_grad()
        pred, target, loss = m.run(wav, mel, voice, jitter)
        loss.backward()
        opt.step()
        want = em.batch(2)
        assert np.array_equal(m._engine.in_wav.cpu().numpy(), want["wav"])          # what the engine saw
        assert np.array_equal(m._engine.in_voice.cpu().numpy(), want["voice"])
        assert bool(torch.isfinite(loss))
