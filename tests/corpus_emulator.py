"""AEW_OP_WINDOW_GATHER restated in numpy / torch (the arithmetic of aew_window_gather_t, include/aewavenet.h): what the
CPU tests hold the recorded reference run (tests/golden/corpus_order.json) and aew_corpus_locate against, and what the
GPU tests hold the kernel against.  Python integers throughout, so no width is ever in play here."""
import numpy as np
import torch

LENGTHS, SLICE, STRIDE = (37, 90, 64, 41, 130, 55), 40, 7            # the golden corpus (make_corpus_golden.py)


def golden_corpus():
    """(snd uint8 [417], samples [(voice, wav_b, wav_e)]): six utterances, voices i % 3."""
    snd = np.random.RandomState(0).randint(0, 256, sum(LENGTHS)).astype(np.uint8)
    samples, at = [], 0
    for i, n in enumerate(LENGTHS):
        samples.append((i % 3, at, at + n))
        at += n
    return snd, samples


def table(samples, slice_size, stride):
    """Rows (start, voice): every stride-th start of an utterance that leaves more than slice_size samples behind it."""
    rows = []
    for voice, b, e in samples:
        s = b
        while s < e - slice_size:
            rows.append((s, voice))
            s += stride
    return rows


def order_row(e, n_order, R, rank):
    gen = torch.Generator()
    gen.manual_seed(e * R + rank)
    return torch.randperm(n_order, generator=gen).tolist()


def locate(t0, b, B, N, n_order, R):
    """(e, p, position epoch, position step) of item b of the batch that starts at t0."""
    e, p = divmod(t0 + b, n_order)
    P = (N + R - 1) // R
    pe, ps = divmod(t0 + B, P)
    return e, p, pe, ps * R


class Emulator:
    def __init__(self, snd, samples, slice_size, stride, R=1, rank=0, start_epoch=0, shuffle=True):
        self.snd, self.n, self.R, self.rank, self.start_epoch, self.shuffle = snd, slice_size, R, rank, start_epoch, shuffle
        self.rows = table(samples, slice_size, stride)
        self.N = len(self.rows)
        self.n_order = len(range(rank, self.N, R))
        self.t = 0
        self._perm = {}

    def perm(self, e):
        if e not in self._perm:
            self._perm[e] = order_row(self.start_epoch + e, self.n_order, self.R, self.rank) if self.shuffle \
                else list(range(self.n_order))
        return self._perm[e]

    def batch(self, B, advance=True):
        """dict(wav float32 [B][n], voice int64 [B], index int32 [B], position int64 [2], starts list)."""
        wav, voice, index, starts = np.zeros((B, self.n), np.float32), [], [], []
        for b in range(B):
            e, p, pe, ps = locate(self.t, b, B, self.N, self.n_order, self.R)
            i = self.rank + self.R * self.perm(e)[p]
            s, v = self.rows[i]
            wav[b] = self.snd[s:s + self.n].astype(np.float32)
            voice.append(v), index.append(i), starts.append(s)
        if advance:
            self.t += B
        return dict(wav=wav, voice=np.asarray(voice, np.int64), index=np.asarray(index, np.int32),
                    position=np.asarray([pe, ps], np.int64), starts=starts)
