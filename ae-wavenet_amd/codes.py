"""Code sequences as data: the functional forms of the two device ops that go with the discrete codes of a VQ-VAE
(csrc/aew_codes.hip), and the mu-law companding that turns an amplitude into the decoder's sample values.

    zq = lookup(emb, codes)                       # AEW_OP_CODE_LOOKUP: codebook rows of a code tensor
    units, lengths, n_runs = code_runs(codes)     # AEW_OP_CODE_RUNS: frames -> units (run-length collapse)
    info = voice_information(codes, voice, K, n_voices)   # AEW_OP_EVAL_GROUPS, codes-only: I(code; voice) of given codes

Both run as one-op plans on torch's current stream, take any device tensor (rows of any length: the concatenated codes
of an utterance) and never synchronise with the host.  `model.encode()` / `model.decode()` / `model.convert()`
(surface.py) are the calls that produce and consume the codes of one window; `model.encode_utterances()` /
`encode_wavs()` / `encode_corpus()` produce those of whole utterances as an `UtteranceCodes`, from the work list
`tile_plan()` states (csrc/aew_utterance.hip); `model.utterance_conditioning()` / `decode_utterances()` /
`convert_utterances()` consume them again at the utterance's length, from the work list `cond_tile_plan()` and the stream
assignment `stream_groups()` (csrc/aew_cond_utterance.hip); `model.score_utterances()` scores a waveform under them with
the teacher-forced decoder, from the work list `score_tile_plan()`, and returns an `UtteranceScores` (csrc/aew_score.hip).
`segment()` chooses the code sequence of whole utterances jointly - penalised Viterbi decoding over the codebook, from the
work list `segment_plan()` (csrc/aew_segment.hip); `model.segment_utterances()` / `segment_wavs()` / `segment_corpus()` are
that call behind the encoder and return an `UtteranceCodes` with a `Segmentation` record.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .plan import pinned_upload


def _run(kind: int, rec, what: str, dev: torch.device):
    if dev.type != "cuda":
        raise L.AewError(f"{what} runs on the GPU only (tensor on '{dev}'); there is no CPU path")
    op = L.Op()
    op.kind = kind
    setattr(op.u, L.OP_FIELD[kind], rec)
    fail = C.c_int(-1)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.load().aew_run_plan(C.byref(op), 1, C.c_void_p(st), C.byref(fail)), what)


def lookup(emb: torch.Tensor, codes: torch.Tensor, d_pitch: Optional[int] = None,
           bad: Optional[torch.Tensor] = None) -> torch.Tensor:
    """emb fp32 (K, d), codes int64 of any shape -> fp32 codes.shape + (d_pitch,), d_pitch = d by default: emb[codes] bit
    for bit, channels d..d_pitch zero.  A code outside [0, K) is not followed: its row is zeros and, with `bad` (an int32
    device tensor; element 0 is the counter, zero it first), counted there."""
    if emb.dim() != 2 or emb.dtype != torch.float32 or codes.dtype != torch.int64:
        raise L.AewError("lookup(): emb fp32 (K, d) and int64 codes expected")
    K, d = emb.shape
    dp = d if d_pitch is None else int(d_pitch)
    emb, flat = emb.contiguous(), codes.to(emb.device).reshape(-1).contiguous()
    zq = torch.empty(flat.numel(), dp, dtype=torch.float32, device=emb.device)
    if flat.numel():
        lk = L.CodeLookup()
        lk.ind, lk.emb, lk.zq, lk.bad = flat.data_ptr(), emb.data_ptr(), zq.data_ptr(), (bad.data_ptr() if bad is not None else None)
        lk.Q, lk.K, lk.d, lk.d_pitch = flat.numel(), K, d, dp
        _run(L.OP_CODE_LOOKUP, lk, "code lookup", emb.device)
    return zq.view(*codes.shape, dp)


def code_runs(codes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """codes int64 (B, N) or (N,) (any row stride) -> (units int64 (B, N), lengths int32 (B, N), n_runs int32 (B,)):
    position t starts a run iff t == 0 or codes[b, t] != codes[b, t - 1]; units[b, r] / lengths[b, r] are the code and the
    length of run r, -1 / 0 behind the last run.  Fixed output sizes - the host is never told a size, so the call can be
    captured in a graph; `units[b, :n_runs[b]]` is the caller's (synchronising) cut."""
    if codes.dtype != torch.int64 or codes.dim() not in (1, 2):
        raise L.AewError("code_runs(): int64 codes (B, N) or (N,) expected")
    one = codes.dim() == 1
    c = codes.unsqueeze(0) if one else codes
    B, N = c.shape
    if c.stride(1) != 1 or (B > 1 and c.stride(0) < N):
        c = c.contiguous()
    units = torch.empty(B, N, dtype=torch.int64, device=c.device)
    lengths = torch.empty(B, N, dtype=torch.int32, device=c.device)
    n_runs = torch.empty(B, dtype=torch.int32, device=c.device)
    cr = L.CodeRuns()
    cr.ind, cr.ind_pitch = c.data_ptr(), (c.stride(0) if B > 1 else N)
    cr.units, cr.lengths, cr.n_runs, cr.B, cr.N = units.data_ptr(), lengths.data_ptr(), n_runs.data_ptr(), B, N
    _run(L.OP_CODE_RUNS, cr, "code runs", c.device)
    return (units[0], lengths[0], n_runs[0]) if one else (units, lengths, n_runs)


def voice_information(codes: torch.Tensor, voice: torch.Tensor, K: int, n_voices: int) -> Dict[str, torch.Tensor]:
    """How much of the voice the codes carry, for codes that come from `model.encode()` or from disk: codes int64
    (B, E) with voice (B,) - one voice per row - or flat (N,) with voice (N,) - one per code; K codebook entries,
    n_voices voices.  One codes-only accumulate (AEW_OP_EVAL_GROUPS) into a fresh record plus one finalize; returns what
    `Evaluator.information()` returns - 0-d float32 device tensors n, code_entropy, group_entropy, cond_entropy,
    mutual_information, mutual_information_mm (Miller-Madow corrected, not clamped), mi_over_group_entropy,
    mi_over_code_entropy, cells, groups_used, codes_used, dropped_windows, batches - plus `counts`, the exact (n_voices, K)
    int64 table.  A code outside [0, K) is not counted; a row whose voice lies outside [0, n_voices) is dropped (and
    counted in dropped_windows).  One workgroup serves one row, so the (B, E) form is the one to use for long
    sequences.  No host synchronisation."""
    if codes.dtype != torch.int64 or codes.dim() not in (1, 2) or codes.numel() < 1:
        raise L.AewError("voice_information(): int64 codes (B, E) or (N,) expected")
    c = codes.unsqueeze(1) if codes.dim() == 1 else codes
    B, E = c.shape
    if tuple(voice.shape) != (B,):
        raise L.AewError(f"voice_information(): voice ({B},) expected (one per row of codes), got {tuple(voice.shape)}")
    K, G = int(K), int(n_voices)
    if K < 1 or G < 1:
        raise L.AewError("voice_information(): K and n_voices must be at least 1")
    dev = c.device
    c, v = c.contiguous(), voice.to(device=dev, dtype=torch.int64).contiguous()
    rec = torch.zeros(G * L.EVAL_GACC_N + 4 + 4 * B + K + 4 * G, dtype=torch.float64, device=dev)   # gacc | gtot | win | scratch
    ghist = torch.zeros(G, K, dtype=torch.int32, device=dev)                                        # (uint32 counts)
    out = torch.empty(G * L.EVAL_GOUT_N + L.EVAL_TOUT_N, dtype=torch.float32, device=dev)
    ev = L.EvalGroups()
    ev.B, ev.ind, ev.Qw, ev.K, ev.group, ev.G = B, c.data_ptr(), E, K, v.data_ptr(), G
    ev.gacc, ev.gtot = rec.data_ptr(), rec.data_ptr() + 8 * G * L.EVAL_GACC_N
    ev.win, ev.scratch = ev.gtot + 8 * 4, ev.gtot + 8 * (4 + 4 * B)
    ev.ghist, ev.gout, ev.tout = ghist.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * G * L.EVAL_GOUT_N
    _run(L.OP_EVAL_GROUPS, ev, "voice information (accumulate)", dev)
    ev.finalize = 1
    _run(L.OP_EVAL_GROUPS, ev, "voice information (finalize)", dev)
    tout = out[G * L.EVAL_GOUT_N:]
    info = {name: tout[i] for i, name in enumerate(L.EVAL_TOUT_NAMES)}
    info["counts"] = ghist.to(torch.int64) & 0xffffffff
    return info


# ---- whole utterances in tiles: what the three work lists (tile_plan, cond_tile_plan, score_tile_plan) share --------------
def _pack_rows(nw: np.ndarray, B: int):
    """Windows per utterance `nw` [U] -> (R, n_rows, utt int32 [R], window int32 [R]): the windows of all utterances, in
    order, fill batches of B rows - n_rows live ones, R rows with the idle ones (utt -1, window 0) that pad the last batch."""
    n_rows = int(nw.sum())
    R = -(-n_rows // B) * B
    utt, window = np.full(R, -1, np.int32), np.zeros(R, np.int32)
    utt[:n_rows] = np.repeat(np.arange(len(nw)), nw)
    window[:n_rows] = np.arange(n_rows) - np.repeat(np.concatenate([[0], np.cumsum(nw)])[:-1], nw)
    return R, n_rows, utt, window


def _live(R: int, n_rows: int, values, dtype) -> np.ndarray:
    """A per-row array [R]: `values` in the n_rows live rows, 0 in the idle ones."""
    out = np.zeros(R, dtype)
    out[:n_rows] = values
    return out


def _code_window(w: np.ndarray, hop: int, p: int, N: np.ndarray, E: int):
    """The code window of windows `w` at a hop of `hop` codes behind `p` pad codes, over utterances of N codes (one per
    window) -> (c0, lo, hi): the window's first code relative to the utterance's, and the window codes [lo, hi) that exist."""
    c0 = w * hop - p
    lo = np.clip(-c0, 0, E)
    return c0, lo, np.maximum(np.clip(N - c0, 0, E), lo)


def _fill_table(rec: np.ndarray, utt: np.ndarray, per_utt: dict, per_row: dict) -> np.ndarray:
    """The live rows of the records `rec`: field = values[utt] for `per_utt` (values one per utterance), field = the row's
    own value for `per_row`; idle rows keep what they hold."""
    live = utt >= 0
    u = utt[live]
    for name, values in per_utt.items():
        rec[name][live] = np.asarray(values, np.int64).reshape(-1)[u]
    for name, values in per_row.items():
        rec[name][live] = values[live]
    return rec


# ---- whole utterances: the work list of model.encode_utterances() and the codes it returns ------------------------------
@dataclass
class TilePlan:
    """tile_plan()'s result: per utterance the code offsets, per batch row (n_batches * B of them, the idle rows that
    fill the last batch included) the utterance (-1: idle), its window, the window's first frame, the frames that exist
    there, the codes stored and where the first of them goes in the flat outputs.  Host arrays only."""
    E: int
    s: int
    rf: int
    mel_len: int
    B: int
    frames: np.ndarray          # int64 [U]
    offsets: np.ndarray         # int64 [U + 1]: utterance u owns codes [offsets[u], offsets[u + 1])
    utt: np.ndarray             # int32 [R]
    window: np.ndarray          # int32 [R]
    start: np.ndarray           # int64 [R]
    avail: np.ndarray           # int32 [R]
    n_valid: np.ndarray         # int32 [R]
    dst: np.ndarray             # int64 [R]
    n_rows: int                 # rows that are not idle

    @property
    def n_batches(self) -> int:
        return len(self.utt) // self.B

    @property
    def n_codes(self) -> int:
        return int(self.offsets[-1])

    def table(self, bases) -> np.ndarray:
        """The aew_utt_row_t records (a structured array, _lib.UTT_ROW_DTYPE) for utterances whose (n_mel, F_u) arrays start
        at the element offsets `bases` [U] of the ragged mel buffer."""
        rec = _fill_table(np.zeros(len(self.utt), np.dtype(L.UTT_ROW_DTYPE)), self.utt, dict(src=bases, pitch=self.frames),
                          dict(dst=self.dst, avail=self.avail, n_valid=self.n_valid))
        rec["src"] += self.start                                             # (0 in idle rows)
        return rec


def tile_plan(frames: Sequence[int], E: int, s: int, rf: int, B: int) -> TilePlan:
    """The work list of a whole-utterance encode, a pure function of the frame counts (it never reads the device): an
    utterance of F frames has N = 0 codes if F < rf, else (F - rf) // s + 1, in ceil(N / E) windows of mel_len =
    s * (E - 1) + rf frames; window w starts at frame w * s * E, finds min(mel_len, F - w * s * E) frames there (the
    rest are zeros) and stores the codes [w * E, min(N, w * E + E)) - those whose receptive field lies inside the real
    frames.  The windows of all utterances, in order, fill batches of B rows; the last batch is padded with idle rows."""
    E, s, rf, B = int(E), int(s), int(rf), int(B)
    if E < 1 or s < 1 or rf < 1 or B < 1:
        raise ValueError("tile_plan(): E, s, rf and B must be at least 1")
    F = np.asarray(list(frames), np.int64).reshape(-1)
    if (F < 0).any():
        raise ValueError("tile_plan(): negative frame count")
    mel_len = s * (E - 1) + rf
    N = np.where(F < rf, 0, (F - rf) // s + 1)
    offsets = np.concatenate([[0], np.cumsum(N)]).astype(np.int64)
    R, n_rows, utt, window = _pack_rows(-(-N // E), B)
    u, w = utt[:n_rows], window[:n_rows].astype(np.int64)
    row = lambda values, dtype=np.int32: _live(R, n_rows, values, dtype)
    return TilePlan(E, s, rf, mel_len, B, F, offsets, utt, window, start=row(w * (s * E), np.int64),
                    avail=row(np.minimum(mel_len, F[u] - w * (s * E))), n_valid=row(np.minimum(E, N[u] - w * E)),
                    dst=row(offsets[u] + w * E, np.int64), n_rows=n_rows)


class UtteranceCodes:
    """The codes of U whole utterances: `codes` int64, flat, on the device; `offsets` int64 (U + 1,) on the host -
    utterance u owns codes[offsets[u]:offsets[u + 1]] (they follow from the frame counts alone, so reading them never
    waits for the device); optional `dist` float32 like codes, `voice` int64 (U,), `names` (U strings)."""

    def __init__(self, codes: torch.Tensor, offsets: torch.Tensor, dist: Optional[torch.Tensor] = None,
                 voice: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None):
        offsets = torch.as_tensor(offsets, dtype=torch.int64).cpu()
        U = offsets.numel() - 1
        if codes.dtype != torch.int64 or codes.dim() != 1 or U < 0 or int(offsets[-1]) != codes.numel() or int(offsets[0]) != 0:
            raise L.AewError("UtteranceCodes: flat int64 codes and offsets (U + 1,) from 0 to len(codes) expected")
        if dist is not None and dist.shape != codes.shape:
            raise L.AewError("UtteranceCodes: dist must have one value per code")
        if voice is not None and tuple(voice.shape) != (U,):
            raise L.AewError(f"UtteranceCodes: voice ({U},) expected, got {tuple(voice.shape)}")
        if names is not None and len(names) != U:
            raise L.AewError(f"UtteranceCodes: {U} names expected, got {len(names)}")
        self.codes, self.offsets, self.dist, self.voice = codes, offsets, dist, voice
        self.names = None if names is None else [str(n) for n in names]
        self._off = offsets.tolist()

    def __len__(self) -> int:
        return len(self._off) - 1

    def row(self, u: int) -> torch.Tensor:
        """The codes of utterance u (a view)."""
        u = range(len(self))[u]
        return self.codes[self._off[u]:self._off[u + 1]]

    def units(self, u: int):
        """codes.code_runs of row u: (units, lengths, n_runs)."""
        return code_runs(self.row(u))

    def padded(self, fill: int = -1) -> torch.Tensor:
        """(U, longest row) int64, row u = its codes followed by `fill`."""
        lens = torch.tensor([b - a for a, b in zip(self._off[:-1], self._off[1:])], dtype=torch.int64)
        width = int(lens.max()) if len(self) else 0
        out = torch.full((len(self), width), int(fill), dtype=torch.int64, device=self.codes.device)
        if self.codes.numel():
            mask = (torch.arange(width)[None, :] < lens[:, None]).to(self.codes.device)
            out.masked_scatter_(mask, self.codes)
        return out

    def save(self, path):
        """One .npz: codes, offsets and - where present - voice, names, dist."""
        arrays = {"codes": self.codes.cpu().numpy(), "offsets": self.offsets.numpy()}
        if self.voice is not None:
            arrays["voice"] = self.voice.cpu().numpy()
        if self.names is not None:
            arrays["names"] = np.asarray(self.names, dtype=np.str_)
        if self.dist is not None:
            arrays["dist"] = self.dist.cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path, device=None) -> "UtteranceCodes":
        with np.load(path, allow_pickle=False) as z:
            put = lambda k: torch.from_numpy(z[k]).to(device) if device is not None else torch.from_numpy(z[k])
            return cls(put("codes"), torch.from_numpy(z["offsets"]), dist=put("dist") if "dist" in z else None,
                       voice=put("voice") if "voice" in z else None,
                       names=[str(n) for n in z["names"]] if "names" in z else None)


# ---- segmenting utterances: the code sequence chosen jointly (csrc/aew_segment.hip) ------------------------------------------
VQ_METRICS = {"scaled_l2": 0, "sq_l2": 1}                  # aew_vq_nearest_t.metric
VQ_METRIC_NAMES = {v: k for k, v in VQ_METRICS.items()}


@dataclass
class SegmentPlan:
    """segment_plan()'s result: the aew_seg_utt_t records (lam left 0 for the caller) of utterances that lie one behind
    the other in the frame buffer, the row offsets and the bytes of workspace one launch over all of them needs."""
    K: int
    offsets: np.ndarray         # int64 [U + 1]: utterance u owns rows (and codes) [offsets[u], offsets[u + 1])
    table: np.ndarray           # _lib.SEG_UTT_DTYPE [U]
    ws_bytes: int

    @property
    def n_frames(self) -> int:
        return int(self.offsets[-1])


def segment_ws_bytes(n_frames: int, K: int) -> int:
    """Bytes of workspace of one AEW_OP_CODE_SEGMENT over n_frames rows: the fp32 local costs, n_frames * K * 4 rounded up
    to 8, then per row ceil(K / 64) + 1 words of back-pointers (aew_segment_ws_bytes states the same)."""
    n, K = int(n_frames), int(K)
    if n < 0 or not 1 <= K <= L.SEG_MAX_K:
        raise ValueError(f"segment_ws_bytes(): n_frames >= 0 and K in [1, {L.SEG_MAX_K}] expected")
    return (n * K * 4 + 7) // 8 * 8 + 8 * n * ((K + 63) // 64 + 1)


def segment_plan(frames_per_utterance: Sequence[int], K: int) -> SegmentPlan:
    """The work list of a segmentation, a pure function of the frame counts (it never reads the device): utterance u owns
    the rows [offsets[u], offsets[u + 1]) and the ceil(K / 64) + 1 back words of each of them, in the same order."""
    n = np.asarray(list(frames_per_utterance), np.int64).reshape(-1)
    if (n < 0).any() or (n >= 1 << 31).any():
        raise ValueError("segment_plan(): frame counts in [0, 2^31) expected")
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ws = segment_ws_bytes(int(offsets[-1]), K)
    t = np.zeros(len(n), dtype=L.SEG_UTT_DTYPE)
    t["first_frame"], t["n_frames"] = offsets[:-1], n
    t["back_base"] = offsets[:-1] * ((int(K) + 63) // 64 + 1)
    return SegmentPlan(int(K), offsets, t, ws)


@dataclass
class Segmentation:
    """What goes with the codes of a segmentation, all on the device: cost (U,) fp32 - the minimum of the objective,
    n_segments (U,) int32 - 1 + the code changes (0 for an empty utterance), penalty (U,) fp32, n_bad int32 (1,) - a
    uint32 count of the utterances whose cost is not finite.  Reading them is the caller's synchronisation."""
    cost: torch.Tensor
    n_segments: torch.Tensor
    penalty: torch.Tensor
    n_bad: torch.Tensor


def _penalties(penalty, U: int, what: str) -> np.ndarray:
    lam = np.asarray(penalty.cpu() if torch.is_tensor(penalty) else penalty, np.float64).reshape(-1)
    if lam.size == 1:
        lam = np.repeat(lam, U)
    if lam.size != U:
        raise L.AewError(f"{what}: penalty must be one number or one per utterance ({U}), got {lam.size}")
    if U and not (lam >= 0).all():                                           # (a NaN fails the comparison)
        raise L.AewError(f"{what}: penalty must be >= 0 (inf is allowed)")
    with np.errstate(over="ignore"):
        return lam.astype(np.float32)


def segment(frames: torch.Tensor, offsets, emb: torch.Tensor, penalty, metric: str = "scaled_l2",
            return_dist: bool = False):
    """Penalised Viterbi decoding of codes on the device (AEW_OP_CODE_SEGMENT; include/aewavenet.h states the rule bit for
    bit): for each utterance the labelling that minimises  sum_t dist(frame t, emb[codes[t]]) + penalty * (code changes).
    frames: fp32 (n, d_pitch) device tensor, contiguous - the utterances' encoder outputs one behind the other, the first
    d channels of a row are read (d = emb.shape[1]; d_pitch >= d); offsets: (U + 1,) host integers from 0 to n; emb fp32
    (K, d), K <= 4096; penalty: one float or one per utterance, >= 0, inf allowed; metric "scaled_l2" or "sq_l2" as in
    the nearest-code search.  penalty 0 gives that search's codes and distances bit for bit; inf gives one code per
    utterance.  -> (codes int64 (n,), cost fp32 (U,), n_seg int32 (U,)), with return_dist=True (codes, dist, cost, n_seg).
    The workspace holds n * K * 4 bytes of local costs.  One launch on torch's current stream, no host synchronisation;
    `segment_full()` also returns the `Segmentation` record."""
    codes, dist, info = segment_full(frames, offsets, emb, penalty, metric, return_dist)
    return (codes, dist, info.cost, info.n_segments) if return_dist else (codes, info.cost, info.n_segments)


def segment_full(frames: torch.Tensor, offsets, emb: torch.Tensor, penalty, metric: str = "scaled_l2",
                 return_dist: bool = False):
    """segment() -> (codes, dist or None, Segmentation)."""
    what = "segment()"
    if metric not in VQ_METRICS:
        raise L.AewError(f"{what}: metric must be one of {sorted(VQ_METRICS)}, got '{metric}'")
    if not torch.is_tensor(frames) or frames.dim() != 2 or frames.dtype != torch.float32 or not frames.is_contiguous():
        raise L.AewError(f"{what}: frames fp32 (n, d_pitch) contiguous expected")
    if emb.dim() != 2 or emb.dtype != torch.float32:
        raise L.AewError(f"{what}: emb fp32 (K, d) expected")
    dev = frames.device
    if dev.type != "cuda" or emb.device != dev:
        raise L.AewError(f"{what} runs on the GPU only (frames on '{dev}', emb on '{emb.device}'); there is no CPU path")
    K, d = emb.shape
    n, d_pitch = frames.shape
    if not 1 <= K <= L.SEG_MAX_K or not 1 <= d <= d_pitch:
        raise L.AewError(f"{what}: K in [1, {L.SEG_MAX_K}] and 1 <= d <= d_pitch expected, got K = {K}, d = {d}, d_pitch = {d_pitch}")
    off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets, np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise L.AewError(f"{what}: offsets (U + 1,) ascending from 0 to {n} expected")
    U = off.size - 1
    plan = segment_plan(np.diff(off), K)
    plan.table["lam"] = _penalties(penalty, U, what)
    emb = emb.contiguous()
    codes = torch.empty(n, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev) if return_dist else None
    cost = torch.empty(U, dtype=torch.float32, device=dev)
    n_seg = torch.empty(U, dtype=torch.int32, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    lam = np.ascontiguousarray(plan.table["lam"])
    info = Segmentation(cost, n_seg, pinned_upload(dev, lam)[0][:lam.nbytes].view(torch.float32), n_bad)
    if U == 0:
        return codes, dist, info
    table, host = pinned_upload(dev, plan.table)
    ws = torch.empty(max(plan.ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    cs = L.CodeSegment()
    cs.frames, cs.n_elems = (frames.data_ptr() if n else None), frames.numel()
    cs.emb, cs.K, cs.d, cs.d_pitch, cs.metric = emb.data_ptr(), K, d, d_pitch, VQ_METRICS[metric]
    cs.table, cs.table_host, cs.U = table.data_ptr(), host.data_ptr(), U
    cs.codes, cs.dist, cs.n_out = codes.data_ptr(), (dist.data_ptr() if dist is not None else None), n
    cs.cost, cs.n_seg, cs.n_bad = cost.data_ptr(), n_seg.data_ptr(), n_bad.data_ptr()
    cs.ws, cs.ws_bytes = ws.data_ptr(), 8 * ws.numel()
    _run(L.OP_CODE_SEGMENT, cs, what, dev)
    # table, host and ws return to torch's allocators, which order their reuse behind this stream's work
    return codes, dist, info


# ---- whole utterances, the other way: the work list of model.utterance_conditioning() / decode_utterances() ------------
@dataclass
class CondTilePlan:
    """cond_tile_plan()'s result: per utterance its conditioning length L(N_u) and its stream; per batch row
    (n_batches * B of them, the idle rows that fill the last batch included) the utterance (-1: idle), its window, the
    window's first code relative to the utterance's (negative in front of it), the window codes [lo, hi) that exist, the
    cond rows [src_row, src_row + n_rows) it owns, the conditioning position dst_row of the first of them and whether it
    is the utterance's first window.  Utterance u is stream u of a [U][pitch][Cp] buffer, pitch = the longest L(N_u)
    (at least 1) unless given; one with L(N_u) = 0 has no row.  Host arrays only."""
    E: int
    S: int
    T: int
    trim0: int
    p: int
    h: int
    B: int
    n_codes: np.ndarray         # int64 [U]
    lengths: np.ndarray         # int64 [U]: L(N_u)
    pitch: int                  # rows per stream
    utt: np.ndarray             # int32 [R]
    window: np.ndarray          # int32 [R]
    start: np.ndarray           # int64 [R]
    lo: np.ndarray              # int32 [R]
    hi: np.ndarray              # int32 [R]
    src_row: np.ndarray         # int32 [R]
    owned: np.ndarray           # int32 [R]: rows the window owns
    dst_row: np.ndarray         # int32 [R]
    first: np.ndarray           # int32 [R]
    n_rows: int                 # rows that are not idle

    @property
    def n_batches(self) -> int:
        return len(self.utt) // self.B

    def offsets(self, Cp: int) -> np.ndarray:
        """Element offset of each utterance's conditioning in the stitched [U][pitch][Cp] buffer."""
        return np.arange(len(self.n_codes), dtype=np.int64) * (self.pitch * int(Cp))

    def table(self, bases, voices) -> np.ndarray:
        """The aew_cond_row_t records (a structured array, _lib.COND_ROW_DTYPE) for utterances whose codes start at the
        indices `bases` [U] of the flat code buffer and whose voices are `voices` [U]."""
        rec = np.zeros(len(self.utt), np.dtype(L.COND_ROW_DTYPE))
        rec["utt"] = -1
        _fill_table(rec, self.utt, dict(code0=bases, voice=voices),
                    dict(utt=self.utt, stream=self.utt, lo=self.lo, hi=self.hi, src_row=self.src_row, n_rows=self.owned,
                         dst_row=self.dst_row, first=self.first, pitch=np.full(len(self.utt), self.pitch)))
        rec["code0"] += self.start                                           # (0 in idle rows)
        return rec


def cond_tile_plan(n_codes: Sequence[int], E: int, S: int, T: int, trim0: int, B: int, L_of, pitch: Optional[int] = None) -> CondTilePlan:
    """The work list of a whole-utterance conditioning, a pure function of the code counts (it never reads the device).
    (E, S, T, trim0) and L_of = n -> L(n) are geometry.conditioning_geometry's: with p = ceil(trim0 / S) pad codes and the
    hop h = (T - (p S - trim0)) // S, an utterance of N codes has ceil(L(N) / (h S)) windows; window w holds the codes
    [w h - p, w h - p + E) - those inside [0, N) exist, the others are code 0 - and owns the conditioning positions
    [w h S, min((w + 1) h S, L(N))): its cond rows from p S - trim0 on.  The windows of all utterances, in order, fill
    batches of B rows; the last batch is padded with idle rows."""
    E, S, T, trim0, B = int(E), int(S), int(T), int(trim0), int(B)
    if E < 1 or S < 1 or T < 1 or trim0 < 0 or B < 1:
        raise ValueError("cond_tile_plan(): E, S, T and B must be at least 1, trim0 at least 0")
    p = -(-trim0 // S)
    lead = p * S - trim0
    h = (T - lead) // S
    if h < 1:
        raise ValueError(f"cond_tile_plan(): T = {T} rows hold no hop of S = {S} behind row {lead}")
    N = np.asarray(list(n_codes), np.int64).reshape(-1)
    if (N < 0).any():
        raise ValueError("cond_tile_plan(): negative code count")
    Ln = np.asarray([int(L_of(int(n))) for n in N], np.int64).reshape(-1)
    if (Ln < 0).any() or (Ln > np.maximum(N, 0) * S).any():
        raise ValueError("cond_tile_plan(): L(n) must lie in [0, n * S]")
    hop = h * S
    R, n_rows, utt, window = _pack_rows(-(-Ln // hop), B)
    t_max = max(int(Ln.max()) if len(Ln) else 0, 1)
    if pitch is None:
        pitch = t_max
    elif int(pitch) < t_max:
        raise ValueError(f"cond_tile_plan(): pitch {pitch} is shorter than the longest conditioning, {t_max} rows")
    u, w = utt[:n_rows], window[:n_rows].astype(np.int64)
    c0, lo, hi = _code_window(w, h, p, N[u], E)
    row = lambda values, dtype=np.int32: _live(R, n_rows, values, dtype)
    return CondTilePlan(E, S, T, trim0, p, h, B, N, Ln, int(pitch), utt, window, start=row(c0, np.int64), lo=row(lo), hi=row(hi),
                        src_row=row(lead), owned=row(np.minimum(hop, Ln[u] - w * hop)), dst_row=row(w * hop), first=row(w == 0),
                        n_rows=n_rows)


def stream_groups(lengths: Sequence[int], seed: int, width: int = 16):
    """Which sampler call generates which utterance, a pure function of (lengths, seed): the utterances with a length
    above 0, ordered longest first (stable: equal lengths keep their input order), are cut into groups of `width`;
    returns [(seed + g, [utterance indices of group g])] - the k-th index of a group is stream slot k of that group's
    one Sampler.generate call, whose seed is seed + g and whose step count is the length of its first member."""
    order = sorted((u for u, n in enumerate(lengths) if int(n) > 0), key=lambda u: -int(lengths[u]))
    return [(int(seed) + g, order[at:at + width]) for g, at in enumerate(range(0, len(order), width))]


# ---- whole utterances through the teacher-forced decoder: the work list and the result of model.score_utterances() ------
@dataclass
class ScoreTilePlan:
    """score_tile_plan()'s result: per utterance n_u (positions that have both a conditioning row and a sample), n_scored
    = max(n_u - rf - 1, 0) and the offsets of its scored samples in the flat outputs; per batch row (n_batches * B of
    them, the idle rows that fill the last batch included) the utterance (-1: idle), its window, the window's first code
    relative to the utterance's, the window codes [lo, hi) that exist, the utterance's sample that is the window's
    decoder-input row 0, the outputs [src, src + n_out) it owns and the flat element the first of them goes to.  Host
    arrays only."""
    E: int
    S: int
    T: int
    rf: int
    r0: int
    p: int
    h_s: int
    o: int
    B: int
    n_codes: np.ndarray         # int64 [U]
    wav_lens: np.ndarray        # int64 [U]
    n_u: np.ndarray             # int64 [U]
    n_scored: np.ndarray        # int64 [U]
    offsets: np.ndarray         # int64 [U + 1]: utterance u owns the flat elements [offsets[u], offsets[u + 1])
    utt: np.ndarray             # int32 [R]
    window: np.ndarray          # int32 [R]
    start: np.ndarray           # int64 [R]
    lo: np.ndarray              # int32 [R]
    hi: np.ndarray              # int32 [R]
    wav0: np.ndarray            # int64 [R]
    src: np.ndarray             # int32 [R]
    n_out: np.ndarray           # int32 [R]
    dst: np.ndarray             # int64 [R]
    n_rows: int                 # rows that are not idle

    @property
    def n_batches(self) -> int:
        return len(self.utt) // self.B

    @property
    def n_total(self) -> int:
        return int(self.offsets[-1])

    def table(self, code_bases, wav_bases, voices) -> np.ndarray:
        """The aew_score_row_t records (a structured array, _lib.SCORE_ROW_DTYPE) for utterances whose codes start at
        the indices `code_bases` [U] of the flat code buffer, whose samples start at the elements `wav_bases` [U] of the
        flat waveform buffer and whose voices are `voices` [U]."""
        rec = np.zeros(len(self.utt), np.dtype(L.SCORE_ROW_DTYPE))
        rec["utt"] = -1
        _fill_table(rec, self.utt, dict(code0=code_bases, wav_base=wav_bases, wav_len=self.wav_lens, voice=voices),
                    dict(utt=self.utt, lo=self.lo, hi=self.hi, wav0=self.wav0, src=self.src, n_out=self.n_out, dst=self.dst))
        rec["code0"] += self.start                                           # (0 in idle rows)
        return rec


def score_tile_plan(n_codes: Sequence[int], wav_lens: Sequence[int], geom_tuple, B: int) -> ScoreTilePlan:
    """The work list of a whole-utterance scoring, a pure function of the code counts and waveform lengths (it never
    reads the device).  geom_tuple = (E, S, T, rf, r0, p, h_s, o, L) is geometry.scoring_geometry(...).plan_args(): utterance
    u has n_u = min(L(N_u), len(wav_u) - o) positions (0 where that is negative) and n_u - rf - 1 scored samples, the
    positions q_t in [rf + 1, n_u); window j holds the codes [j h_s - p, j h_s - p + E) - those inside [0, N) exist, the
    others are code 0 -, its decoder-input row 0 is the utterance's sample o + j h_s S - r0, and it owns the outputs
    [r0, r0 + h_s S) whose target j h_s S + (u - r0) + rf + 1 lies below n_u; there are ceil((n_u - rf - 1) / (h_s S))
    windows.  The windows of all utterances, in order, fill batches of B rows; the last batch is padded with idle rows."""
    E, S, T, rf, r0, p, h_s, o = (int(v) for v in tuple(geom_tuple)[:8])
    L_of, B = tuple(geom_tuple)[8], int(B)
    if E < 1 or S < 1 or T < 1 or rf < 0 or r0 < 0 or p < 0 or o < 0 or B < 1:
        raise ValueError("score_tile_plan(): E, S, T and B must be at least 1, rf, r0, p and o at least 0")
    if h_s < 1 or r0 + h_s * S > T - rf - 1:
        raise ValueError(f"score_tile_plan(): the {T} - {rf} - 1 outputs of a window that carry a loss do not hold a hop of "
                         f"h_s = {h_s} codes of S = {S} behind output {r0}")
    N = np.asarray(list(n_codes), np.int64).reshape(-1)
    W = np.asarray(list(wav_lens), np.int64).reshape(-1)
    if len(N) != len(W) or (N < 0).any() or (W < 0).any():
        raise ValueError("score_tile_plan(): one non-negative code count and one waveform length per utterance expected")
    Ln = np.asarray([int(L_of(int(n))) for n in N], np.int64).reshape(-1)
    if (Ln < 0).any() or (Ln > np.maximum(N, 0) * S).any():
        raise ValueError("score_tile_plan(): L(n) must lie in [0, n * S]")
    n_u = np.maximum(np.minimum(Ln, W - o), 0)
    n_sc = np.maximum(n_u - rf - 1, 0)
    offsets = np.concatenate([[0], np.cumsum(n_sc)]).astype(np.int64)
    hop = h_s * S
    R, n_rows, utt, window = _pack_rows(-(-n_sc // hop), B)
    u, j = utt[:n_rows], window[:n_rows].astype(np.int64)
    c0, lo, hi = _code_window(j, h_s, p, N[u], E)
    row = lambda values, dtype=np.int32: _live(R, n_rows, values, dtype)
    return ScoreTilePlan(E, S, T, rf, r0, p, h_s, o, B, N, W, n_u, n_sc, offsets, utt, window, start=row(c0, np.int64), lo=row(lo),
                         hi=row(hi), wav0=row(o + j * hop - r0, np.int64), src=row(r0), n_out=row(np.minimum(hop, n_sc[u] - j * hop)),
                         dst=row(offsets[u] + j * hop, np.int64), n_rows=n_rows)


class UtteranceScores:
    """The teacher-forced likelihood of U whole utterances (model.score_utterances): `nll` float32, flat, on the device -
    utterance u owns nll[offsets[u]:offsets[u + 1]], n_scored[u] values, and row(u)[i] is the NLL in nats of waveform
    sample start + i of that utterance (start = o + rf + 1); `prob` (the probability given to the sample that came) and
    `hit` (uint8: the arg-max class was the sample) alike where they were asked for; `offsets` int64 (U + 1,) and
    `n_scored` int64 (U,) on the device (their host copies follow from the lengths alone: reading row() never waits);
    `summary` float32 (U, 4) = (nll per sample, bits per sample, top-1, mean target probability) and `sums` float64
    (U, 4) = (n, sum nll, sum prob, sum hit), summed in a fixed order that depends neither on the batch nor on the
    tiling; `voice` int64 (U,) on the host.  An utterance with nothing to score has an empty row and a zero summary."""

    def __init__(self, nll: torch.Tensor, offsets, summary: torch.Tensor, sums: torch.Tensor, start: int,
                 prob: Optional[torch.Tensor] = None, hit: Optional[torch.Tensor] = None, voice=None):
        off = torch.as_tensor(offsets, dtype=torch.int64).cpu()
        U = off.numel() - 1
        if nll.dim() != 1 or nll.dtype != torch.float32 or U < 0 or int(off[0]) != 0 or int(off[-1]) != nll.numel():
            raise L.AewError("UtteranceScores: flat float32 nll and offsets (U + 1,) from 0 to len(nll) expected")
        if tuple(summary.shape) != (U, 4) or tuple(sums.shape) != (U, 4):
            raise L.AewError(f"UtteranceScores: summary and sums ({U}, 4) expected")
        for name, t in (("prob", prob), ("hit", hit)):
            if t is not None and t.shape != nll.shape:
                raise L.AewError(f"UtteranceScores: {name} must have one value per scored sample")
        self._off = off.tolist()
        self.nll, self.prob, self.hit, self.summary, self.sums, self.start = nll, prob, hit, summary, sums, int(start)
        self.offsets = off.to(nll.device)
        self.n_scored = (off[1:] - off[:-1]).to(nll.device)
        self.voice = None if voice is None else torch.as_tensor(voice, dtype=torch.int64).cpu().reshape(-1)

    def __len__(self) -> int:
        return len(self._off) - 1

    def _cut(self, t, u):
        u = range(len(self))[u]
        return t[self._off[u]:self._off[u + 1]]

    def row(self, u: int) -> torch.Tensor:
        """The per-sample NLL of utterance u in nats (a view): element i belongs to waveform sample start + i."""
        return self._cut(self.nll, u)

    def prob_row(self, u: int) -> torch.Tensor:
        return self._cut(self.prob, u)

    def hit_row(self, u: int) -> torch.Tensor:
        return self._cut(self.hit, u)

    # the columns of `summary` as (U,) views, one accessor per name of _lib.SCORE_OUT_NAMES (attached behind the class)

    def save(self, path):
        """One .npz: nll, offsets, summary, sums, start and - where present - prob, hit, voice."""
        arrays = {"nll": self.nll.cpu().numpy(), "offsets": np.asarray(self._off, np.int64), "summary": self.summary.cpu().numpy(),
                  "sums": self.sums.cpu().numpy(), "start": np.asarray(self.start, np.int64)}
        for name in ("prob", "hit", "voice"):
            if getattr(self, name) is not None:
                arrays[name] = getattr(self, name).cpu().numpy()
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path, device=None) -> "UtteranceScores":
        with np.load(path, allow_pickle=False) as z:
            put = lambda k: torch.from_numpy(z[k]).to(device) if device is not None else torch.from_numpy(z[k])
            return cls(put("nll"), torch.from_numpy(z["offsets"]), put("summary"), put("sums"), int(z["start"]),
                       prob=put("prob") if "prob" in z else None, hit=put("hit") if "hit" in z else None,
                       voice=torch.from_numpy(z["voice"]) if "voice" in z else None)


def _summary_column(i: int, name: str):
    return property(lambda self: self.summary[:, i], doc=f"`summary[:, {i}]`: {name} of every utterance, a (U,) view.")


for _i, _name in enumerate(L.SCORE_OUT_NAMES):                            # nll_per_sample, bits_per_sample, top1, mean_prob
    setattr(UtteranceScores, _name, _summary_column(_i, _name))


# ---- mu-law companding of the decoder's samples (amplitudes in [-1, 1] -> n_quant integer values) ---------------------
def mu_encode(x: torch.Tensor, n_quant: int = 256) -> torch.Tensor:
    """Amplitudes in [-1, 1] -> int64 mu-law values in [0, n_quant): with mu = n_quant - 1, the compressed amplitude
    sign(x) ln(1 + mu |x|) / ln(1 + mu) is mapped affinely onto [0, mu] and rounded to the nearest integer (halves up)."""
    mu = float(n_quant - 1)
    y = torch.sign(x) * torch.log1p(mu * x.abs()) / math.log1p(mu)
    return torch.floor((y + 1.0) * (0.5 * mu) + 0.5).to(torch.int64).clamp_(0, n_quant - 1)


def mu_decode(x: torch.Tensor, n_quant: int = 256) -> torch.Tensor:
    """mu-law values in [0, n_quant) (any integer or float dtype) -> float32 amplitudes in [-1, 1], the inverse of
    mu_encode: with mu = n_quant - 1 and y = 2 x / mu - 1, sign(y) ((1 + mu)^|y| - 1) / mu.  mu_encode(mu_decode(v)) = v
    for every value v."""
    mu = float(n_quant - 1)
    y = x.to(torch.float32) * (2.0 / mu) - 1.0
    return torch.sign(y) * torch.expm1(y.abs() * math.log1p(mu)) / mu

