#!/usr/bin/env python3
"""Generate tests/golden/corpus_order.json by RUNNING the reference's data pipeline.

Runs only where the reference is at hand (its directory in AEW_REFERENCE; it never travels to the GPU box).
What is written is recorded results only: for R = 1 rank 0 and R = 3 ranks 0, 1, 2, the (slice start, voice, epoch, step)
of every item of 12 batches of 4 that the reference's own SliceDataset, TrackerDataset and LoopingRandomSampler deliver
under DataLoader(num_workers=0, batch_size=4).  Re-run with

    AEW_REFERENCE=<the reference's directory> python -B tests/golden/make_corpus_golden.py

Shims (the reference's code is not changed):
  1. the empty stub modules of make_golden.py for tensorboard / tensorboardX / librosa / fire;
  2. LoopingRandomSampler.__init__ raises under the installed torch (Sampler.__init__ takes no argument any more), so
     the sampler is made with object.__new__ and its four attributes are set; only its __iter__ is the subject;
  3. a pass-through dataset between TrackerDataset and SliceDataset notes which row of in_start every item is, so the
     slice start can be recorded (the slice's bytes are checked against snd_data[start : start + slice_size] here).

The corpus: six utterances of 37, 90, 64, 41, 130, 55 samples, voices i % 3, slice_size 40, n_win_batch 7 (N = 29),
bytes numpy.random.RandomState(0).randint(0, 256, 417).
"""
import contextlib
import io
import json
import os
import pickle
import sys
import tempfile
import types

sys.dont_write_bytecode = True
REF = os.environ.get("AEW_REFERENCE")
if not REF or not os.path.exists(os.path.join(REF, "data.py")):
    sys.exit("set AEW_REFERENCE to the directory that holds the reference's data.py")
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

for name in ("tensorboard", "torch.utils.tensorboard", "tensorboardX", "librosa", "fire"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.SummaryWriter = object
        sys.modules[name] = m
sys.path.insert(0, REF)

import data             # noqa: E402

LENGTHS, SLICE, STRIDE, BATCH, N_BATCHES = (37, 90, 64, 41, 130, 55), 40, 7, 4, 12


class Spy(Dataset):
    def __init__(self, inner):
        self.inner = inner

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, item):
        snd, voice = self.inner[item]
        return snd, voice, item


def run(dat_path, snd, R, rank):
    slices = data.SliceDataset(SLICE, STRIDE)
    slices.load_data(dat_path)
    tracker = data.TrackerDataset(Spy(slices), 0, 0, sampling_freq=R)
    sampler = object.__new__(data.LoopingRandomSampler)
    sampler.dataset, sampler.num_replicas, sampler.rank, sampler.epoch = tracker, R, rank, 0
    loader = DataLoader(tracker, sampler=sampler, num_workers=0, batch_size=BATCH, pin_memory=False,
                        collate_fn=lambda batch: batch)
    batches = []
    with contextlib.redirect_stderr(io.StringIO()):
        it = iter(loader)
        for _ in range(N_BATCHES):
            rec = []
            for (got, voice, item), epoch, step in next(it):
                start, v = slices.in_start[item]
                assert v == voice and np.array_equal(got, snd[start:start + SLICE])
                rec.append([int(start), int(voice), int(epoch), int(step)])
            batches.append(rec)
    return {"num_replicas": R, "rank": rank, "n_slices": len(slices), "batches": batches}


def main():
    snd = np.random.RandomState(0).randint(0, 256, sum(LENGTHS)).astype(np.uint8)
    samples, at = [], 0
    for i, n in enumerate(LENGTHS):
        samples.append(data.SpokenSample(voice_index=i % 3, wav_b=at, wav_e=at + n, file_path=f"utt{i}.wav"))
        at += n
    with tempfile.TemporaryDirectory() as tmp:
        dat_path = os.path.join(tmp, "corpus.dat")
        with open(dat_path, "wb") as fh:
            pickle.dump({"samples": samples, "snd_dtype": np.uint8, "snd_data": snd}, fh)
        runs = [run(dat_path, snd, R, rank) for R, rank in ((1, 0), (3, 0), (3, 1), (3, 2))]
    out = {"lengths": list(LENGTHS), "slice_size": SLICE, "n_win_batch": STRIDE, "batch_size": BATCH,
           "item": ["slice start", "voice", "epoch", "step"], "runs": runs}
    with open(os.path.join(HERE, "corpus_order.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote corpus_order.json:", [(r["num_replicas"], r["rank"], r["n_slices"]) for r in runs])


if __name__ == "__main__":
    main()
