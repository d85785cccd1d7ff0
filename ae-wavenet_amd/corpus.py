"""The training corpus held in device memory, batches cut out of it on the device (reference: data.py
`SliceDataset`, `LoopingRandomSampler`, `TrackerDataset` under a `DataLoader`, a Python loop per item on the host).

    corpus = DeviceCorpus.from_dat("librispeech.dat", slice_size, hps.n_win_batch, "cuda:0", num_replicas=R, rank=r)
    batches = DeviceBatches(corpus, hps.n_batch, mfcc=DeviceMfcc("cuda:0"), jitter=DeviceJitter(0.12, seed))
    for wav, mel, voice, jitter, position in batches:
        pred, target, loss = model.run(wav, mel, voice, jitter)

The corpus is uploaded once; every batch is ONE op (AEW_OP_WINDOW_GATHER, aew_window_gather_t in aewavenet.h) that reads
how many items this rank has consumed from a device counter, follows the sampler's permutation and the reference's
`in_start` table, and writes the windows as the float tensor the reference's collate function builds (data.py:229), the
speakers, the table rows used and the `(epoch, step)` the reference's TrackerDataset reports.  No host work per batch
beyond issuing the op, no host synchronisation, replayable from a captured graph (`gather_op`, `note_batches`).

Order.  The row of sampler epoch e is `torch.randperm(n_order, generator=g)` with `g.manual_seed((start_epoch + e) * R +
rank)` on the CPU - the call of data.py:99-103 - so the order of batches is the reference's by construction.  Two rows are
resident (a batch may straddle two epochs); the host keeps a deterministic mirror of the device counter and, before the
first batch that starts in epoch e, copies the row of e + 1 into slot (e + 1) & 1 - last read by epoch e - 1, which is
behind on the same stream - without blocking, from a pinned buffer.

Resume.  `state_dict()` / `load_state_dict()` carry the number of items consumed; a resumed corpus yields exactly the
batches the uninterrupted run would have, bit for bit.  THE REFERENCE DOES SOMETHING DIFFERENT: after a restart its
sampler replays the epoch's permutation from its beginning (only the epoch number is restored), so the items between
the epoch's start and the checkpoint are seen twice.

`start_epoch` shifts the sampler's seed epoch only, as LoopingRandomSampler's constructor argument does; `position`
counts from (0, 0) like a fresh TrackerDataset.

No CPU path: with `device=None` only the host tables and the mirror exist (what the tests without a GPU look at) and
every method that would touch the device raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import pickle
from collections import deque, namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L

SpokenSample = namedtuple("SpokenSample", ["voice_index", "wav_b", "wav_e", "file_path"])     # (data.py:78-84)

_SND_DTYPES = (np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.int32))                     # (data.py:35-40)
_SLACK = 16                    # bytes readable past the last element (aew_window_gather_t's contract)


class _DatUnpickler(pickle.Unpickler):
    """The reference's .dat pickle and nothing else: its SpokenSample records, and the names numpy needs to rebuild an
    array and a dtype.  Any other global raises."""
    _NUMPY = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
              ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
              ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy", "uint8"), ("numpy", "int16"), ("numpy", "int32")}

    def find_class(self, module, name):
        if (module, name) == ("data", "SpokenSample"):
            return SpokenSample
        if (module, name) in self._NUMPY:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"corpus file names the global {module}.{name}: refused")


def read_dat(path):
    """(snd_data, samples) of a file written by the reference's data.convert()."""
    with open(path, "rb") as fh:
        dat = _DatUnpickler(fh).load()
    if not isinstance(dat, dict) or not {"samples", "snd_dtype", "snd_data"} <= set(dat):
        raise ValueError(f"{path}: not a corpus file (samples / snd_dtype / snd_data expected)")
    return np.asarray(dat["snd_data"]).astype(dat["snd_dtype"]), list(dat["samples"])


def slice_table(samples: Sequence, slice_size: int, n_win_batch: int):
    """The reference's `in_start` (SliceDataset.load_data, data.py:173-176) as (starts int64 [N], voices int32 [N]):
    per utterance, in catalogue order, the starts range(wav_b, wav_e - slice_size, n_win_batch)."""
    starts, voices = [], []
    for sam in samples:
        voice, wav_b, wav_e = int(sam[0]), int(sam[1]), int(sam[2])
        r = range(wav_b, wav_e - slice_size, n_win_batch)
        starts.extend(r)
        voices.extend([voice] * len(r))
    return np.asarray(starts, np.int64), np.asarray(voices, np.int32)


def permutation_row(epoch: int, n_order: int, num_replicas: int, rank: int) -> torch.Tensor:
    """The sampler's permutation of this rank's slice list in (seed) epoch `epoch` (data.py:99-103), int32 [n_order]."""
    g = torch.Generator()
    g.manual_seed(epoch * num_replicas + rank)
    return torch.randperm(n_order, generator=g).to(torch.int32)


class _Cursor:
    """One consumer's place in the corpus: the two resident order rows, the device counter and its host mirror.
    `items` mirrors the device counter (batches issued), `consumed` counts the batches handed to the caller - the two
    differ only while a DeviceBatches with prefetch holds batches it has produced ahead.  `stream`: where this cursor's
    device work runs (None: the caller's current stream)."""

    def __init__(self, corpus: "DeviceCorpus", shuffle: bool):
        self.c, self.shuffle, self.items, self.consumed = corpus, shuffle, 0, 0
        self.stream, self.generation = None, 0        # generation: bumped by seek(), batches produced before it are stale
        self.order = self.counter = None
        self._resident = None                         # slots hold the rows of sampler epochs _resident and _resident + 1
        if corpus.device is not None:
            n = corpus.n_order
            self.order = torch.zeros(2, n, dtype=torch.int32, device=corpus.device)
            self.counter = torch.zeros(1, dtype=torch.int64, device=corpus.device)      # (the op reads it as uint64)
            self._pinned = torch.empty(2, n, dtype=torch.int32, pin_memory=True)
            self._ev = [None, None]
            self.seek(0)

    def row(self, e: int) -> torch.Tensor:
        c = self.c
        if not self.shuffle:
            return torch.arange(c.n_order, dtype=torch.int32)
        return permutation_row(c.start_epoch + e, c.n_order, c.num_replicas, c.rank)

    def _upload(self, e: int):
        slot = e & 1
        if self._ev[slot] is not None:                # the copy that read this pinned row last (an epoch ago) is done
            self._ev[slot].synchronize()
        np.copyto(self._pinned[slot].numpy(), self.row(e).numpy())     # (plain host memcpy: see loader.DevicePrefetcher)
        with self.on_stream():
            self.order[slot].copy_(self._pinned[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
        self._ev[slot] = ev

    @contextlib.contextmanager
    def on_stream(self):
        with torch.cuda.device(self.c.device):
            if self.stream is None:
                yield
            else:
                with torch.cuda.stream(self.stream):
                    yield

    def seek(self, items: int):
        """Continue at `items` consumed: counter, mirror and the two rows that place needs."""
        self.items = self.consumed = int(items)
        self.generation += 1
        if self.counter is None:
            return
        e = self.items // self.c.n_order
        with self.on_stream():
            self.counter.fill_(self.items)
        self._upload(e)
        self._upload(e + 1)
        self._resident = e

    def before_batch(self):
        """Issued in front of the batch that starts at the mirror's place: the first batch to start in sampler epoch e
        brings the row of e + 1 into slot (e + 1) & 1."""
        if self.counter is None:
            self.c._need_device()
        e = self.items // self.c.n_order
        if e == self._resident:
            return False
        assert e == self._resident + 1, "a batch is never longer than a sampler epoch"
        if self.shuffle:                              # (the held-out order is the identity in every row)
            self._upload(e + 1)
        self._resident = e
        return True

    def position(self):
        """TrackerDataset's (epoch, step) after the `consumed` items (the closed form of aew_window_gather_t)."""
        c = self.c
        P = -(-c.N // c.num_replicas)
        return self.consumed // P, (self.consumed % P) * c.num_replicas


class DeviceCorpus:
    def __init__(self, snd_data, samples: Sequence, slice_size: int, n_win_batch: int, device, num_replicas: int = 1,
                 rank: int = 0, start_epoch: int = 0):
        """snd_data: 1-D uint8 / int16 / int32 array of mu-law values; samples: (voice_index, wav_b, wav_e[, ...])
        records, the reference's SpokenSample; device: a cuda device, or None for the host tables alone."""
        snd = np.ascontiguousarray(snd_data)
        if snd.ndim != 1 or snd.dtype not in _SND_DTYPES:
            raise TypeError("snd_data: 1-D uint8, int16 or int32 expected (data.py:35-40)")
        if slice_size < 1 or n_win_batch < 1:
            raise ValueError("slice_size >= 1 and n_win_batch >= 1")
        if num_replicas < 1 or not 0 <= rank < num_replicas:
            raise ValueError("rank in [0, num_replicas)")
        self.samples = list(samples)
        self.slice_size, self.n_win_batch = int(slice_size), int(n_win_batch)
        self.num_replicas, self.rank, self.start_epoch = int(num_replicas), int(rank), int(start_epoch)
        self.snd_host, self.n_snd, self.snd_bytes = snd, int(snd.shape[0]), int(snd.dtype.itemsize)
        self.starts_host, self.voices_host = slice_table(self.samples, self.slice_size, self.n_win_batch)
        self.N = int(self.starts_host.shape[0])
        self.n_order = len(range(self.rank, self.N, self.num_replicas))
        if self.n_order < 1:
            raise ValueError(f"no slice for rank {rank} of {num_replicas}: the corpus yields {self.N} slices")
        if int(self.starts_host.min()) < 0 or int(self.starts_host.max()) + self.slice_size > self.n_snd:
            raise ValueError("a sample's (wav_b, wav_e) leaves snd_data")
        self.device = None if device is None else torch.device(device)
        self.snd = self.starts = self.voices = None
        if self.device is not None:
            if self.device.type != "cuda":
                raise L.AewError("DeviceCorpus holds the corpus on an MI355X (device=None: host tables only)")
            L.load()
            raw = snd.view(np.uint8)
            padded = -(-(raw.shape[0] + _SLACK) // 16) * 16
            self.snd = torch.zeros(padded, dtype=torch.uint8, device=self.device)     # (allocations are 512-byte aligned)
            self.snd[:raw.shape[0]].copy_(torch.from_numpy(raw))
            self.starts = torch.from_numpy(self.starts_host).to(self.device)
            self.voices = torch.from_numpy(self.voices_host).to(self.device)
        self.cursor = _Cursor(self, shuffle=True)
        self._B = None

    @classmethod
    def from_arrays(cls, snd_data, samples, slice_size, n_win_batch, device, **kw) -> "DeviceCorpus":
        """The constructor under the name that pairs with from_dat."""
        return cls(snd_data, samples, slice_size, n_win_batch, device, **kw)

    @classmethod
    def from_dat(cls, path, slice_size: int, n_win_batch: int, device, num_replicas: int = 1, rank: int = 0,
                 start_epoch: int = 0) -> "DeviceCorpus":
        """From the file the reference's data.convert() writes, read with a restricted unpickler (no reference import)."""
        snd, samples = read_dat(path)
        return cls(snd, samples, slice_size, n_win_batch, device, num_replicas, rank, start_epoch)

    def num_speakers(self) -> int:
        return max(int(s[0]) for s in self.samples) + 1

    def __len__(self) -> int:
        return self.N

    def _need_device(self):
        raise L.AewError("this DeviceCorpus holds host tables only (device=None); batches are cut on an MI355X")

    # ---- the op ---------------------------------------------------------------------------------
    def gather_op(self, B: int, wav: torch.Tensor, voice: torch.Tensor, index: torch.Tensor, position: torch.Tensor,
                  advance: int = 1, cursor: Optional[_Cursor] = None) -> L.Op:
        """The AEW_OP_WINDOW_GATHER record for a caller's own plan or captured graph: wav float32 [B][pitch] (pitch a
        multiple of 4, >= slice_size), voice int64 [B], index int32 [B], position int64 [2].  A caller that replays it
        itself tells the mirror with note_batches()."""
        if self.device is None:
            self._need_device()
        cur = cursor or self.cursor
        if wav.dtype != torch.float32 or wav.dim() != 2 or wav.shape[0] < B or wav.stride(1) != 1 or \
                voice.dtype != torch.int64 or index.dtype != torch.int32 or position.dtype != torch.int64 or \
                voice.numel() < B or index.numel() < B or position.numel() < 2:
            raise ValueError("gather_op: wav float32 [B][pitch], voice int64 [B], index int32 [B], position int64 [2]")
        g = L.WindowGather()
        g.snd, g.n_snd, g.snd_bytes, g.B = self.snd.data_ptr(), self.n_snd, self.snd_bytes, B
        g.starts, g.voices, g.N = self.starts.data_ptr(), self.voices.data_ptr(), self.N
        g.order, g.n_order, g.num_replicas, g.rank = cur.order.data_ptr(), self.n_order, self.num_replicas, self.rank
        g.advance, g.counter = int(bool(advance)), cur.counter.data_ptr()
        g.slice_size, g.wav_pitch = self.slice_size, wav.stride(0)
        g.wav, g.voice, g.index, g.position = wav.data_ptr(), voice.data_ptr(), index.data_ptr(), position.data_ptr()
        op = L.Op()
        op.kind = L.OP_WINDOW_GATHER
        op.u.wgat = g
        if cur is self.cursor:
            self._B = B
        return op

    def note_batches(self, n: int = 1, batch_size: Optional[int] = None):
        """For a caller that replays a graph holding gather_op(advance=1): account for the next `n` replays of
        `batch_size` items (default: the B of the last gather_op) BEFORE they are launched, on the stream they run on.
        A row upload belongs directly in front of the batch that needs it, so only the first of the n batches may be
        the first of a sampler epoch: call it per replay (n = 1) where that cannot be ruled out."""
        B = self._B if batch_size is None else int(batch_size)
        if B is None:
            raise ValueError("note_batches: no batch size (gather_op has not been called)")
        for k in range(n):
            if self.cursor.items // self.n_order != self.cursor._resident and k > 0:
                raise L.AewError("note_batches: a later batch of the n starts a sampler epoch; note the replays one by one")
            self.cursor.before_batch()
            self.cursor.items += B
            self.cursor.consumed = self.cursor.items

    # ---- resume ---------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return {"items": self.cursor.consumed, "num_replicas": self.num_replicas, "rank": self.rank, "n_slices": self.N,
                "start_epoch": self.start_epoch}

    def load_state_dict(self, state: dict):
        """Continue where `state` was taken: the batches that follow are those of the uninterrupted run, bit for bit
        (the reference restarts the epoch's permutation instead, see the module docstring)."""
        for key, mine in (("num_replicas", self.num_replicas), ("rank", self.rank), ("n_slices", self.N)):
            if int(state[key]) != mine:
                raise ValueError(f"corpus state was taken with {key} = {state[key]}, this corpus has {mine}")
        if int(state["items"]) < 0:
            raise ValueError("corpus state: items < 0")
        self.start_epoch = int(state.get("start_epoch", self.start_epoch))
        self.cursor.seek(int(state["items"]))


class DeviceBatches:
    """Iterator over (wav, mel, voice, jitter, position), the reference's training tuple (data.py:237), every tensor on
    the device: wav float32 (B, slice_size), mel from `mfcc` (a DeviceMfcc) or None, voice int64 (B,), jitter from
    `jitter` (a DeviceJitter; `jitter_frames` where no mel gives the number of frames) or None, position int64 (2,).
    `.position` is the same (epoch, step) as Python ints from the host mirror, `.index` the int32 rows of in_start used.

    shuffle=True: endless, the sampler's order, shared with the corpus (its state_dict() follows these batches).
    shuffle=False: the held-out form for model.evaluate() - one pass over the rank's slices in in_start order with a
    place of its own, the final short batch included (the reference's test loader has drop_last=False), then
    StopIteration; reset() starts the pass again.

    prefetch=0: the op, the MFCC and the jitter launches of a batch are issued on the caller's stream when the batch is
    asked for.  prefetch=k: they run on a stream of this iterator's own, k batches ahead, beside the caller's step (what
    DevicePrefetcher does with its copy stream); a batch is handed over through an event, without a host
    synchronisation.  `.position`, `.index` and the corpus' state_dict() always speak of the batches HANDED OUT; after a
    load_state_dict() or reset() the batches produced ahead are dropped.  With prefetch the place's device work moves to
    that stream, so gather_op() in a caller's own graph wants a corpus of its own."""

    def __init__(self, corpus: DeviceCorpus, batch_size: int, mfcc=None, jitter=None, shuffle: bool = True,
                 jitter_frames: Optional[int] = None, prefetch: int = 0):
        if corpus.device is None:
            corpus._need_device()
        if not 1 <= batch_size <= corpus.n_order:
            raise ValueError(f"batch_size in [1, {corpus.n_order}] (a batch is never longer than a sampler epoch)")
        if jitter is not None and mfcc is None and jitter_frames is None:
            raise ValueError("jitter without mfcc needs jitter_frames")
        if prefetch < 0:
            raise ValueError("prefetch >= 0")
        self.corpus, self.B, self.mfcc, self.jitter, self.shuffle = corpus, int(batch_size), mfcc, jitter, shuffle
        self.jitter_frames, self.prefetch = jitter_frames, int(prefetch)
        self.cursor = corpus.cursor if shuffle else _Cursor(corpus, shuffle=False)
        if self.prefetch and self.cursor.stream is None:
            with torch.cuda.device(corpus.device):
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())           # behind the uploads the place has issued so far
            self.cursor.stream = side
        self.index = None
        self._pitch = -(-corpus.slice_size // 4) * 4
        self._q, self._gen = deque(), self.cursor.generation

    @property
    def position(self):
        return self.cursor.position()

    def reset(self):
        if self.shuffle:
            raise ValueError("the training order has no beginning to return to (load_state_dict sets its place)")
        self.cursor.seek(0)

    def __iter__(self):
        return self

    def _produce(self) -> bool:
        c, cur, B = self.corpus, self.cursor, self.B
        if not self.shuffle:
            B = min(B, c.n_order - cur.items)
            if B <= 0:
                return False
        dev = c.device
        with cur.on_stream():
            cur.before_batch()
            wav = torch.empty(B, self._pitch, dtype=torch.float32, device=dev)
            voice = torch.empty(B, dtype=torch.int64, device=dev)
            index = torch.empty(B, dtype=torch.int32, device=dev)
            position = torch.empty(2, dtype=torch.int64, device=dev)
            ops = (L.Op * 1)(c.gather_op(B, wav, voice, index, position, cursor=cur))
            fail = C.c_int(-1)
            st = torch.cuda.current_stream().cuda_stream
            L.check(L.load().aew_run_plan(C.cast(ops, C.c_void_p), 1, C.c_void_p(st), C.byref(fail)), "window gather")
            cur.items += B
            wav = wav[:, :c.slice_size]
            mel = self.mfcc(wav) if self.mfcc is not None else None
            jit = None
            if self.jitter is not None:
                jit = self.jitter(B, mel.shape[2] if mel is not None else self.jitter_frames, dev)
            ev = None
            if cur.stream is not None:
                ev = torch.cuda.Event()
                ev.record(cur.stream)
        self._q.append(((wav, mel, voice, jit, position), index, cur.items, ev))
        return True

    def __next__(self):
        cur = self.cursor
        if self._gen != cur.generation:                  # the place was moved: what was produced ahead is stale
            self._q.clear()
            self._gen = cur.generation
        if not self._q and not self._produce():
            raise StopIteration
        items, index, consumed, ev = self._q.popleft()
        if ev is not None:                               # the caller's stream continues behind the producer's work
            mine = torch.cuda.current_stream(self.corpus.device)
            mine.wait_event(ev)
            for x in items + (index,):
                if x is not None:
                    x.record_stream(mine)
        cur.consumed, self.index = consumed, index
        while len(self._q) < self.prefetch and self._produce():
            pass
        return items
