"""Comparing utterances on the device: dynamic time warping over sequences of feature frames and the edit distance of
code strings, thousands of independent pairs per launch (AEW_OP_SEQ_ALIGN, csrc/aew_align.hip; include/aewavenet.h
states the rule bit for bit).

    al = dtw(a, b)                          # a, b: Ragged views or lists of (n_u, D) fp32 device tensors; pair u = (a[u], b[u])
    al.cost, al.steps, al.mean              # device tensors (P,): summed local distance, path length, cost / steps
    al = dtw(a, pairs=[(0, 1), (0, 2)], return_path=True);  al.path(0)      # (steps, 2) int32 cells - the ONE call that waits
    ed = edit_distance(codes_a, codes_b, collapse=True);    ed.distance, ed.rate
    err = abx(d_ax, d_bx)                   # ABX error of paired distances, a device scalar
    mt = search(queries, docs, pairs=..., n_hits=3)         # subsequence DTW (AEW_OP_SEQ_SEARCH, csrc/aew_search.hip)
    mt.start, mt.end, mt.cost, mt.steps, mt.mean, mt.count  # (P, n_hits): where each query occurs, best first; mt.profile(p)
    rp = discover(utts, threshold=0.5, n_hits=3, min_len=5) # local-alignment DTW (AEW_OP_SEQ_DISCOVER, csrc/aew_discover.hip)
    rp.a_start, rp.a_end, rp.b_start, rp.b_end, rp.score    # (P, n_hits): which stretches of a pair repeat each other
    dist = distance_matrix(items)                           # (N, N) fp32: every pair i < j through dtw(), mirrored, diagonal 0
    res = abx_score(dist, category, speaker, mode="within") # ABX discriminability of the item set (AEW_OP_ABX_COUNT,
    res.error, res.pooled, res.by_category, res.n_triples   # csrc/aew_abx.hip); abx_task(items, ...) is the two in one call

`model.code_distance()` and `model.cepstral_distance()` (surface.py) are these calls over the codebook rows of code
sequences and over the model's own MFCC front-end; `model.search_codes()` and `model.search_wavs()` are `search` over the
same two feature sources, `model.discover_codes()` and `model.discover_wavs()` are `discover`.  On the device dtw() and
search() run one sweep (`align_sweep` in csrc/aew_align.hip), discover() its sibling over the same ring of local
distances, search() and discover() one pick (`seq_pick`), all three one sweep-and-second-kernel launch, and here the
three ops share one launch path, `_SeqPlan`: it checks the two sides, fills the record
fields the ops have in common and runs the records as a plan on torch's current stream (`_run_records`, abx_score()'s
way too); search() and discover() share what lies on top of it - the pair table, the launch (`_HitsLaunch`), the result
(`_Hits`) and the argument checks; the workspace of each op follows from `CELL_WORDS`.  Every host table (and
edit_distance()'s denominator) goes up through `_upload` - pinned, behind the stream.  Nothing
but `Alignment.path()` (and `edit_distance(collapse=True)`, which has to learn the number of units) synchronises with
the host.  There is no CPU path: a tensor that is not on the GPU is refused.

ABX over an item set.  `abx_tables` turns the labels into the three host tables of the op (a pure host function),
`abx_score` uploads them through `_upload`, runs the op as a one-record plan and hands its integer counts to
`abx_aggregate`, which is pure torch, dense throughout (no step has a data-dependent size, nothing synchronises) and
therefore also runs on CPU tensors.  The aggregation: the counts of every X are pooled inside a (category of X, category
of B, speaker of X, speaker of A and B) cell; a cell with triples has the error wrong2 / (2 n); `by_category[cX][cB]` is
the plain mean of the cells of that category pair over the speaker combinations present, and `error` the plain mean of
`by_category` over its present ORDERED pairs - so neither a frequent category nor a talkative speaker weighs more than
another.  With mode "within" (A, B and X of one speaker) and "across" (A and B of one speaker, X of another) these are
the usual within- and across-speaker ABX scores without a context ("by") label: fold a context into `category` to get
one.  `pooled` is every triple in one pool.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .plan import pinned_upload

METRICS = {"euclid": L.ALIGN_EUCLID, "sqeuclid": L.ALIGN_SQEUCLID}
STRIP = 64                                   # A frames a wave holds at a time: longer A sides carry a boundary row in the workspace
# int32 words that travel with the fp32 value of a cell, per op (AEW_*_WORDS in csrc/aew_align.hip): a boundary row takes
# 1 + CELL_WORDS planes of pairs * wstride 4-byte words in the workspace
CELL_WORDS = {"align": 1, "search": 2, "discover": 3}


def _metric_of(what: str, metric: str) -> int:
    if metric not in METRICS:
        raise L.AewError(f"{what}: metric must be one of {sorted(METRICS)}, got '{metric}'")
    return METRICS[metric]


class Ragged:
    """Sequences inside ONE device buffer, read in place: element (i, k) of sequence u is
    flat[base[u] + i * frame_stride[u] + k * chan_stride[u]], i < length[u], k < D.  frame_stride / chan_stride: one int
    for all sequences or one per sequence.  Frame-major (n, D) rows are (frame_stride, chan_stride) = (D, 1); the
    channel-major (channels, frames) arrays of `DeviceMfcc.ragged` are (1, frames) - with `base` moved by c0 * frames
    and a smaller D the view takes channels c0 .. c0 + D - 1 only."""

    def __init__(self, flat: torch.Tensor, base: Sequence[int], length: Sequence[int], frame_stride, chan_stride, D: int):
        U = len(base)
        one = lambda v: [int(v)] * U if np.isscalar(v) else [int(x) for x in v]
        self.flat, self.D = flat, int(D)
        self.base, self.length = [int(x) for x in base], [int(x) for x in length]
        self.frame_stride, self.chan_stride = one(frame_stride), one(chan_stride)
        if not torch.is_tensor(flat) or flat.dim() != 1 or not flat.is_contiguous():
            raise L.AewError("Ragged: a flat contiguous tensor expected")
        if not (len(self.length) == len(self.frame_stride) == len(self.chan_stride) == U):
            raise L.AewError("Ragged: base, length and the strides must have one entry per sequence")
        n = flat.numel()
        for u in range(U):
            ln, fs, cs, b = self.length[u], self.frame_stride[u], self.chan_stride[u], self.base[u]
            if ln < 0 or ln > L.ALIGN_MAX_LEN or fs < 0 or cs < 0:
                raise L.AewError(f"Ragged: sequence {u}: length in [0, {L.ALIGN_MAX_LEN}] and strides >= 0 expected")
            if ln and (b < 0 or b + (ln - 1) * fs + (self.D - 1) * cs >= n):
                raise L.AewError(f"Ragged: sequence {u} reaches outside its buffer of {n} elements")

    def __len__(self) -> int:
        return len(self.base)

    def table(self) -> np.ndarray:
        """The aew_align_seq_t records."""
        t = np.zeros(len(self), dtype=L.ALIGN_SEQ_DTYPE)
        t["base"], t["len"] = self.base, self.length
        t["frame_stride"], t["chan_stride"] = self.frame_stride, self.chan_stride
        return t


def _ragged(x, what: str, dtype) -> Ragged:
    """A Ragged as it is; a list of (n_u, D) tensors (dtype fp32) or 1-D tensors (int64) concatenated once."""
    if isinstance(x, Ragged):
        if x.flat.dtype != dtype:
            raise L.AewError(f"{what}: a {dtype} buffer expected, got {x.flat.dtype}")
        return x
    rows = list(x)
    want = 2 if dtype == torch.float32 else 1
    for r in rows:
        if not torch.is_tensor(r) or r.dim() != want or r.dtype != dtype:
            raise L.AewError(f"{what}: a Ragged or a list of {'(n, D) float32' if want == 2 else '1-D int64'} tensors expected")
    if not rows:
        raise L.AewError(f"{what}: at least one sequence expected")
    if len({r.device for r in rows}) != 1:
        raise L.AewError(f"{what}: the sequences lie on different devices")
    D = int(rows[0].shape[1]) if want == 2 else 1
    if want == 2 and any(int(r.shape[1]) != D for r in rows):
        raise L.AewError(f"{what}: every sequence must have the same number of channels")
    lens = [int(r.shape[0]) for r in rows]
    base = [0]
    for ln in lens:
        base.append(base[-1] + ln * D)
    flat = torch.cat([r.reshape(-1) for r in rows])
    return Ragged(flat, base[:-1], lens, D, 1, D)


def default_pairs(n_a: int, n_b: Optional[int], pairs) -> np.ndarray:
    """(P, 2) int64: `pairs` as given, else (u, u) for every u - zip(a, b), which needs as many b as a."""
    if pairs is None:
        if n_b is not None and n_b != n_a:
            raise L.AewError(f"without pairs= the two sides are zipped: {n_a} and {n_b} sequences do not match")
        u = np.arange(n_a, dtype=np.int64)
        return np.stack([u, u], 1)
    pr = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or pr.shape[0] < 1 or not np.issubdtype(pr.dtype, np.integer):
        raise L.AewError("pairs: a (P, 2) integer array with P >= 1 expected")
    pr = pr.astype(np.int64)
    nb = n_a if n_b is None else n_b
    if (pr < 0).any() or (pr[:, 0] >= n_a).any() or (pr[:, 1] >= nb).any():
        raise L.AewError(f"pairs: an index outside the {n_a} / {nb} sequences")
    return pr


def pair_table(lens_a: Sequence[int], lens_b: Sequence[int], pairs: np.ndarray, max_back_bytes: Optional[int]):
    """(records, chunks, n_back, n_path, wstride).  records: aew_align_pair_t with path_base = the prefix sum of
    n + m - 1 over ALL pairs and back_base = the prefix sum of n * m inside the pair's chunk; chunks: [(lo, hi)] runs of
    consecutive pairs whose back matrices fit max_back_bytes together (one run with max_back_bytes None; a pair larger
    than the limit gets a run of its own); n_back: bytes the largest chunk needs; n_path: path entries of all pairs;
    wstride: per chunk, the longest B side among its pairs of more than STRIP A frames (the workspace is
    4 * (1 + CELL_WORDS["align"]) * pairs * wstride bytes).  A pair with an empty side owns neither back bytes nor path entries."""
    P = len(pairs)
    la, lb = np.asarray(lens_a, np.int64)[pairs[:, 0]], np.asarray(lens_b, np.int64)[pairs[:, 1]]
    live = (la > 0) & (lb > 0)
    cells, cap = np.where(live, la * lb, 0), np.where(live, la + lb - 1, 0)
    t = np.zeros(P, dtype=L.ALIGN_PAIR_DTYPE)
    t["a"], t["b"] = pairs[:, 0], pairs[:, 1]
    t["path_base"] = np.concatenate([[0], np.cumsum(cap)[:-1]])
    chunks, lo, held = [], 0, 0
    for p in range(P):
        if max_back_bytes is not None and p > lo and held + int(cells[p]) > int(max_back_bytes):
            chunks.append((lo, p))
            lo, held = p, 0
        t["back_base"][p] = held
        held += int(cells[p])
    chunks.append((lo, P))
    n_back = max(int(cells[a:b].sum()) for a, b in chunks)
    wstride = [int(np.where(la[a:b] > STRIP, lb[a:b], 0).max()) for a, b in chunks]
    return t, chunks, n_back, int(cap.sum()), wstride


def _upload(table: np.ndarray, dev) -> torch.Tensor:
    """The bytes of a host table on the device (plan.pinned_upload: the host does not wait)."""
    return pinned_upload(dev, table)[0]


def _run_records(dev, kind: int, field: str, recs, what: str):
    """Records of one kind as one plan on torch's current stream of `dev`; a failure names `what` and the record."""
    fail = C.c_int(-1)
    ops = (L.Op * len(recs))()
    for op, r in zip(ops, recs):
        op.kind = kind
        setattr(op.u, field, r)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.load().aew_run_plan(C.cast(ops, C.c_void_p), len(recs), C.c_void_p(st), C.byref(fail)), what,
                fail.value if fail.value >= 0 else None)


class _SeqPlan:
    """The launch path dtw() / edit_distance() (`_Launches`), search() (`_SearchLaunch`) and discover()
    (`_DiscoverLaunch`) share: the checks of the two sides, the three tables, the fields aew_seq_align_t,
    aew_seq_search_t and aew_seq_discover_t have in common, the workspace's size, the run as one plan."""
    KIND, FIELD, NOUN = None, None, None

    def _open(self, ra: Ragged, rb: Ragged):
        dev = ra.flat.device
        if rb.flat.device != dev:
            raise L.AewError(f"the two sides lie on different devices ('{dev}' and '{rb.flat.device}')")
        if ra.D != rb.D:
            raise L.AewError(f"the two sides have {ra.D} and {rb.D} channels")
        if not 1 <= ra.D <= L.ALIGN_MAX_D:
            raise L.AewError(f"D must lie in [1, {L.ALIGN_MAX_D}], got {ra.D}")
        if dev.type != "cuda":
            raise L.AewError(f"the {self.NOUN} runs on the GPU only (tensor on '{dev}'); there is no CPU path")
        self.dev, self.sides, self.recs = dev, (ra, rb), []
        return dev

    def _tables(self, tp: np.ndarray):
        self.host = (self.sides[0].table(), self.sides[1].table(), tp)   # the launcher reads these at every launch
        self.tables = tuple(_upload(t, self.dev) for t in self.host)     # uploaded once per call

    def _workspace(self, pairs_by_wstride: int):
        """The boundary rows of the largest launch: pairs * wstride cells (None: no A side is longer than STRIP)."""
        n = (1 + CELL_WORDS[self.FIELD]) * pairs_by_wstride
        return torch.empty(n, dtype=torch.float32, device=self.dev) if n else None

    def _add(self, r, ws, lo: int = 0):
        """Record r, its common fields filled (the pair table from record `lo` on), joins the plan."""
        (ra, rb), (ta, tb, tp) = self.sides, self.host
        r.seq_a, r.seq_a_host, r.n_a = self.tables[0].data_ptr(), ta.ctypes.data, len(ta)
        r.seq_b, r.seq_b_host, r.n_b = self.tables[1].data_ptr(), tb.ctypes.data, len(tb)
        r.pairs, r.pairs_host = self.tables[2].data_ptr() + lo * tp.itemsize, tp.ctypes.data + lo * tp.itemsize
        r.feat_a, r.n_feat_a = (ra.flat.data_ptr() if ra.flat.numel() else None), ra.flat.numel()
        r.feat_b, r.n_feat_b = (rb.flat.data_ptr() if rb.flat.numel() else None), rb.flat.numel()
        if ws is not None:
            r.ws, r.ws_bytes = ws.data_ptr(), 4 * ws.numel()
        self.recs.append(r)

    def run(self, what: str):
        _run_records(self.dev, self.KIND, self.FIELD, self.recs, what)
        return self


class _Launches(_SeqPlan):
    """The op records of one call and everything they point to."""
    KIND, FIELD, NOUN = L.OP_SEQ_ALIGN, "align", "alignment"

    def __init__(self, mode: int, metric: int, ra: Ragged, rb: Ragged, pairs: np.ndarray, want_path: bool,
                 max_back_bytes: Optional[int]):
        dev = self._open(ra, rb)
        P = self.P = len(pairs)
        self.want_path = want_path
        tp, self.chunks, n_back, self.n_path, wstride = pair_table(ra.length, rb.length, pairs,
                                                                   max_back_bytes if want_path else None)
        self._tables(tp)
        self.cost = torch.empty(P, dtype=torch.float32, device=dev)
        self.steps = torch.empty(P, dtype=torch.int32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = self._workspace(max((b - a) * w for (a, b), w in zip(self.chunks, wstride)))
        self.back = torch.empty(max(n_back, 1), dtype=torch.uint8, device=dev) if want_path else None
        self.path = torch.empty(max(self.n_path, 1), 2, dtype=torch.int32, device=dev) if want_path else None
        self.path_base = tp["path_base"].copy()
        for lo, hi in self.chunks:
            r = L.SeqAlign()
            r.mode, r.metric, r.D, r.n_pairs = mode, metric, ra.D, hi - lo
            r.cost, r.steps, r.bad = self.cost.data_ptr() + 4 * lo, self.steps.data_ptr() + 4 * lo, self.bad.data_ptr()
            if want_path:
                r.back, r.n_back = self.back.data_ptr(), self.back.numel()
                r.path, r.n_path = self.path.data_ptr(), self.path.shape[0]
            self._add(r, self.ws, lo)


class Alignment:
    """What dtw() returns.  cost (P,) fp32: the local distances summed along the best path (+inf for a pair with an empty
    side, NaN for one with a non-finite local distance); steps (P,) int32: the cells on that path (0 for those pairs);
    mean = cost / steps; bad: int32 (1,), a uint32 count of the pairs that were not finite.  All on the device; reading
    them is the caller's synchronisation."""

    def __init__(self, run: _Launches):
        self.cost, self.steps, self.bad = run.cost, run.steps, run.bad
        self.mean = run.cost / run.steps
        self._run = run

    def __len__(self) -> int:
        return self._run.P

    def path(self, p: int) -> torch.Tensor:
        """The warping path of pair p: (steps, 2) int32 cells (i, j) from (0, 0) to (n - 1, m - 1), on the device.  This
        call - and no other here - waits for the device: it reads steps[p] to cut the pair's fixed-size path region."""
        if not self._run.want_path:
            raise L.AewError("path(): the alignment was computed without return_path=True")
        p = range(len(self))[p]
        n = int(self.steps[p].item())
        lo = int(self._run.path_base[p])
        return self._run.path[lo:lo + n]


def dtw(a, b=None, pairs=None, metric: str = "euclid", return_path: bool = False, max_back_bytes: int = 1 << 30) -> Alignment:
    """Dynamic time warping of pairs of sequences of D-channel fp32 frames (D <= 256).  a, b: `Ragged` views or lists of
    (n_u, D) float32 device tensors (concatenated once); b=None compares `a` with itself.  pairs: (P, 2) integers, pair p
    = (a[pairs[p, 0]], b[pairs[p, 1]]), default zip(a, b).  metric "euclid" or "sqeuclid": the local distance.  The step
    pattern is the symmetric one - diagonal, up, left, each of weight 1, ties in that order - with no band.
    return_path=True keeps one back-pointer byte per cell; when those of all pairs exceed max_back_bytes the pairs run in
    several launches that share one buffer of bounded size (the tables are uploaded once).  -> `Alignment`."""
    metric = _metric_of("dtw()", metric)
    ra = _ragged(a, "dtw(): a", torch.float32)
    rb = ra if b is None else _ragged(b, "dtw(): b", torch.float32)
    pr = default_pairs(len(ra), None if b is None else len(rb), pairs)
    return Alignment(_Launches(L.ALIGN_DTW, metric, ra, rb, pr, bool(return_path), int(max_back_bytes)).run("dtw()"))


RANKS = {"mean": L.SEARCH_MEAN, "cost": L.SEARCH_COST}


def _hit_limits(what: str, n_hits, min_len, max_len) -> Tuple[int, int, int]:
    """n_hits, min_len and max_len of search() / discover() as integers, checked."""
    n_hits, min_len, max_len = int(n_hits), int(min_len), int(max_len)
    if not 1 <= n_hits <= L.SEARCH_MAX_HITS:
        raise L.AewError(f"{what}: n_hits must lie in [1, {L.SEARCH_MAX_HITS}], got {n_hits}")
    if min_len < 0 or max_len < 0:
        raise L.AewError(f"{what}: min_len and max_len must not be negative, got {min_len} and {max_len}")
    return n_hits, min_len, max_len


def _profile_pair_table(dtype, lens_a: Sequence[int], lens_b: Sequence[int], pairs: np.ndarray, owner: int, band=None):
    """(records, n_prof, wstride) of search() and discover().  records: `dtype` with prof_base = the prefix sum, over
    the pairs in order, of the lengths of the side that owns the profile (0: A, 1: B) - disjoint profile ranges - and,
    where the record has one, the pair's band; n_prof: their total; wstride: the longest B side among the pairs whose A
    side has more than STRIP frames."""
    la, lb = np.asarray(lens_a, np.int64)[pairs[:, 0]], np.asarray(lens_b, np.int64)[pairs[:, 1]]
    own = (la, lb)[owner]
    t = np.zeros(len(pairs), dtype=dtype)
    t["a"], t["b"] = pairs[:, 0], pairs[:, 1]
    if band is not None:
        t["band"] = band
    t["prof_base"] = np.concatenate([[0], np.cumsum(own)[:-1]])
    return t, int(own.sum()), int(np.where(la > STRIP, lb, 0).max())


def search_pair_table(lens_q: Sequence[int], lens_d: Sequence[int], pairs: np.ndarray):
    """(records, n_prof, wstride).  records: aew_search_pair_t with prof_base = the prefix sum of the document lengths over
    the pairs in order (disjoint profile ranges); n_prof: their total; wstride: the longest document among the pairs whose
    query has more than STRIP frames (the workspace is 4 * (1 + CELL_WORDS["search"]) * pairs * wstride bytes)."""
    return _profile_pair_table(L.SEARCH_PAIR_DTYPE, lens_q, lens_d, pairs, 1)


def discover_pair_table(lens_a: Sequence[int], lens_b: Sequence[int], pairs: np.ndarray, band: np.ndarray):
    """(records, n_prof, wstride).  records: aew_discover_pair_t with prof_base = the prefix sum of the A lengths over the
    pairs in order (disjoint profile ranges) and the pair's band; n_prof: their total; wstride: the longest B side among
    the pairs whose A side has more than STRIP frames (the workspace is 4 * (1 + CELL_WORDS["discover"]) * pairs * wstride
    bytes)."""
    return _profile_pair_table(L.DISCOVER_PAIR_DTYPE, lens_a, lens_b, pairs, 0, band)


class _HitsLaunch(_SeqPlan):
    """The op record of one search or one discovery and everything it points to: the profile arrays `prof` (the first
    fp32, the others int32), the hits (P, n_hits, HIT_WORDS), their `score` (search: the cost) and steps, count, bad, the
    workspace; prof_base and own_len cut a pair's profile without a wait.  A subclass names the record (REC), its fields
    (PROF, and SCORE for `score`), the side whose lengths the profiles have (OWNER; 0: A, 1: B) and its pair table."""
    REC, PROF, SCORE, HIT_WORDS, OWNER = None, (), None, None, None

    def __init__(self, ra: Ragged, rb: Ragged, pairs: np.ndarray, table, n_hits: int, **fields):
        dev = self._open(ra, rb)
        P = self.P = len(pairs)
        tp, n_prof, wstride = table
        self._tables(tp)
        self.prof = tuple(torch.empty(max(n_prof, 1), dtype=torch.int32 if k else torch.float32, device=dev)
                          for k in range(len(self.PROF)))
        self.hits = torch.empty(P, n_hits, self.HIT_WORDS, dtype=torch.int32, device=dev)
        self.score = torch.empty(P, n_hits, dtype=torch.float32, device=dev)
        self.steps = torch.empty(P, n_hits, dtype=torch.int32, device=dev)
        self.count = torch.empty(P, dtype=torch.int32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = self._workspace(P * wstride)
        self.prof_base = tp["prof_base"].copy()
        self.own_len = np.asarray((ra, rb)[self.OWNER].length, np.int64)[pairs[:, self.OWNER]]
        r = self.REC()
        r.D, r.n_pairs, r.n_hits, r.n_prof = ra.D, P, n_hits, n_prof
        for name, value in fields.items():
            setattr(r, name, value)
        for name, x in zip(self.PROF + ("hits", self.SCORE, "hit_steps", "count", "bad"),
                           self.prof + (self.hits, self.score, self.steps, self.count, self.bad)):
            setattr(r, name, x.data_ptr())
        self._add(r, self.ws)


class _Hits:
    """What `Matches` and `Repeats` share: steps (P, n_hits) and count (P,) int32, bad, the number of pairs, profile()."""

    def __init__(self, run: _HitsLaunch):
        self.steps, self.count, self.bad, self._run = run.steps, run.count, run.bad, run

    def __len__(self) -> int:
        return self._run.P

    def profile(self, p: int):
        """The profile of pair p, as the class text names it: views of the pair's range in every profile array.  The
        lengths come from the host tables: no wait on the device."""
        p = range(len(self))[p]
        lo, n = int(self._run.prof_base[p]), int(self._run.own_len[p])
        return tuple(x[lo:lo + n] for x in self._run.prof)


class _SearchLaunch(_HitsLaunch):
    KIND, FIELD, NOUN, REC = L.OP_SEQ_SEARCH, "search", "search", L.SeqSearch
    PROF, SCORE, HIT_WORDS, OWNER = ("prof_cost", "prof_steps", "prof_start"), "hit_cost", 2, 1

    def __init__(self, metric: int, rank: int, rq: Ragged, rd: Ragged, pairs: np.ndarray, n_hits: int, min_len: int,
                 max_len: int):
        super().__init__(rq, rd, pairs, search_pair_table(rq.length, rd.length, pairs), n_hits,
                         metric=metric, rank=rank, min_len=min_len, max_len=max_len)


class Matches(_Hits):
    """What search() returns.  start, end (P, n_hits) int32: the document frames [start, end] of hit r of pair p, best
    first, (-1, -1) behind the `count[p]` hits that exist; cost (P, n_hits) fp32 (+inf there), steps (P, n_hits) int32
    (0 there), mean = cost / steps; count (P,) int32; bad: int32 (1,), a uint32 count of the pairs that were not finite.
    All on the device; reading them is the caller's synchronisation.

    profile(p) -> (end_cost, end_steps, end_start) of pair p: views of length m, entry j the best match that ENDS at
    document frame j - its summed distance, its path length and the frame it starts at ((NaN, 0, -1) for a pair that was
    not finite, (+inf, 0, -1) for an empty query)."""

    def __init__(self, run: _SearchLaunch):
        super().__init__(run)
        self.start, self.end, self.cost = run.hits[:, :, 0], run.hits[:, :, 1], run.score
        self.mean = run.score / run.steps


def search(query, doc=None, pairs=None, metric: str = "euclid", n_hits: int = 1, rank: str = "mean", min_len: int = 1,
           max_len: int = 0) -> Matches:
    """Where does a query occur inside a document: subsequence DTW (AEW_OP_SEQ_SEARCH) of pairs of sequences of D-channel
    fp32 frames.  query, doc: `Ragged` views or lists of (n_u, D) float32 device tensors, exactly as for dtw() (doc=None
    searches `query` in itself); pairs (P, 2) integers, pair p = (query[pairs[p, 0]], doc[pairs[p, 1]]), default zip.
    The whole query is matched against ANY stretch of the document under dtw()'s step pattern and local distance; the
    n_hits (1 .. 32) best stretches that do not overlap are returned best first, ranked by "mean" (cost / steps) or
    "cost".  A match may collapse onto very few document frames - min_len / max_len (document frames, max_len 0: no
    limit) bound the stretches that count.  Nothing here synchronises with the host.  -> `Matches`."""
    metric = _metric_of("search()", metric)
    if rank not in RANKS:
        raise L.AewError(f"search(): rank must be one of {sorted(RANKS)}, got '{rank}'")
    n_hits, min_len, max_len = _hit_limits("search()", n_hits, min_len, max_len)
    rq = _ragged(query, "search(): query", torch.float32)
    rd = rq if doc is None else _ragged(doc, "search(): doc", torch.float32)
    pr = default_pairs(len(rq), None if doc is None else len(rd), pairs)
    return Matches(_SearchLaunch(metric, RANKS[rank], rq, rd, pr, n_hits, min_len, max_len).run("search()"))


def discover_pairs(n_a: int, n_b: Optional[int], pairs) -> np.ndarray:
    """(P, 2) int64: `pairs` as given; else, for one list (n_b None), every unordered pair u <= v INCLUDING (u, u) in
    row-major order, and for two lists zip(a, b) as everywhere here."""
    if pairs is None and n_b is None:
        u, v = np.triu_indices(n_a)
        return np.stack([u, v], 1).astype(np.int64)
    return default_pairs(n_a, n_b, pairs)


class _DiscoverLaunch(_HitsLaunch):
    KIND, FIELD, NOUN, REC = L.OP_SEQ_DISCOVER, "discover", "discovery", L.SeqDiscover
    PROF, SCORE, HIT_WORDS, OWNER = ("prof_score", "prof_end", "prof_row", "prof_col", "prof_steps"), "hit_score", 4, 0

    def __init__(self, metric: int, threshold: float, ra: Ragged, rb: Ragged, pairs: np.ndarray, band: np.ndarray,
                 n_hits: int, min_len: int, max_len: int):
        self.threshold = threshold
        super().__init__(ra, rb, pairs, discover_pair_table(ra.length, rb.length, pairs, band), n_hits,
                         metric=metric, threshold=threshold, min_len=min_len, max_len=max_len)


class Repeats(_Hits):
    """What discover() returns.  a_start, a_end, b_start, b_end (P, n_hits) int32: hit r of pair p aligns the frames
    [a_start, a_end] of its A side with the frames [b_start, b_end] of its B side, best first, -1 behind the `count[p]`
    hits that exist; score (P, n_hits) fp32: the summed gains threshold - d along the alignment (NaN there); steps
    (P, n_hits) int32: its cells (0 there); mean = threshold - score / steps: the mean local distance along it; count
    (P,) int32; bad: int32 (1,), a uint32 count of the pairs that were not finite.  All on the device; reading them is
    the caller's synchronisation.

    profile(p) -> (score, end, origin_row, origin_col, steps) of pair p: views of length n, entry i the best local
    alignment that ENDS in row i of the A side - its score E(i), the B frame it ends at, the (A, B) frames it starts at and
    its cells; (0, -1, -1, -1, 0) where nothing ends, (NaN, -1, -1, -1, 0) for a pair that was not finite."""

    def __init__(self, run: _DiscoverLaunch):
        super().__init__(run)
        self.a_start, self.a_end, self.b_start, self.b_end = (run.hits[:, :, k] for k in range(4))
        self.score = run.score
        self.mean = run.threshold - run.score / run.steps


def discover(a, b=None, pairs=None, threshold: Optional[float] = None, metric: str = "euclid", n_hits: int = 3,
             min_len: int = 1, max_len: int = 0, band: Optional[int] = None) -> Repeats:
    """Which stretches of two utterances say the same thing: local-alignment DTW (AEW_OP_SEQ_DISCOVER) of pairs of
    sequences of D-channel fp32 frames - nobody names a query, an alignment may start and end at any cell.  a, b:
    `Ragged` views or lists of (n_u, D) float32 device tensors as for dtw().  b=None compares `a` with itself over every
    unordered pair u <= v INCLUDING (u, u) - a repeat inside one utterance; with b, or with pairs (P, 2) integers, pair
    p = (a[pairs[p, 0]], b[pairs[p, 1]]), default zip.  A cell gains threshold - d(i, j) (metric as in dtw()): frames
    closer than `threshold` extend an alignment, farther ones wear it down, and it ends where its score would fall to
    zero.  The n_hits (1 .. 32) best alignments whose A ranges do not overlap are returned best first; both spans of a
    hit are at least min_len and, with max_len > 0, at most max_len frames.  A pair (u, u) of one list skips the cells
    with j - i < band - the trivial diagonal and the lower triangle; the default band is max(min_len, 1), an explicit
    band= replaces it, every other pair has band 0.  Nothing here synchronises with the host.  -> `Repeats`."""
    metric = _metric_of("discover()", metric)
    with np.errstate(over="ignore"):
        finite = threshold is not None and bool(np.isfinite(np.float32(threshold)))
    if not finite:
        raise L.AewError(f"discover(): a finite threshold is needed, got {threshold}")
    n_hits, min_len, max_len = _hit_limits("discover()", n_hits, min_len, max_len)
    self_band = max(min_len, 1) if band is None else int(band)
    if not 0 <= self_band < 1 << 31:
        raise L.AewError(f"discover(): band must not be negative, got {band}")
    ra = _ragged(a, "discover(): a", torch.float32)
    rb = ra if b is None else _ragged(b, "discover(): b", torch.float32)
    pr = discover_pairs(len(ra), None if b is None else len(rb), pairs)
    bands = np.where(pr[:, 0] == pr[:, 1], self_band, 0) if rb is ra else np.zeros(len(pr), np.int64)
    return Repeats(_DiscoverLaunch(metric, float(np.float32(threshold)), ra, rb, pr, bands, n_hits, min_len,
                                   max_len).run("discover()"))


class EditDistances:
    """What edit_distance() returns: distance (P,) int32 and rate (P,) fp32 = distance / max(len_a, len_b) (0 where both
    are empty) on the device; len_a / len_b (P,) the compared lengths (host)."""

    def __init__(self, distance, rate, len_a, len_b):
        self.distance, self.rate, self.len_a, self.len_b = distance, rate, len_a, len_b

    def __len__(self) -> int:
        return int(self.distance.numel())


def _symbol_rows(x, what: str) -> list:
    from . import codes as CD
    rows = [x.row(u) for u in range(len(x))] if isinstance(x, CD.UtteranceCodes) else list(x)
    for r in rows:
        if not torch.is_tensor(r) or r.dim() != 1 or r.dtype != torch.int64:
            raise L.AewError(f"{what}: an UtteranceCodes or a list of 1-D int64 tensors expected")
    if not rows:
        raise L.AewError(f"{what}: at least one sequence expected")
    if len({r.device for r in rows}) != 1:
        raise L.AewError(f"{what}: the sequences lie on different devices")
    if rows[0].device.type != "cuda":
        raise L.AewError(f"{what}: the alignment runs on the GPU only (tensor on '{rows[0].device}'); there is no CPU path")
    return rows


def _units(rows: list) -> Ragged:
    """The run-length units of every row (codes.code_runs) as one Ragged; one read of the run counts."""
    from . import codes as CD
    dev = rows[0].device
    parts, counts = [], []
    for r in rows:
        if r.numel():
            units, _, n_runs = CD.code_runs(r)
            parts.append(units)
            counts.append(n_runs.reshape(1))
        else:
            counts.append(torch.zeros(1, dtype=torch.int32, device=dev))
    lens = torch.cat(counts).cpu().tolist()
    base = [0]
    for r in rows:
        base.append(base[-1] + int(r.numel()))
    flat = torch.cat(parts) if parts else torch.zeros(1, dtype=torch.int64, device=dev)
    return Ragged(flat, base[:-1], lens, 1, 1, 1)


def edit_distance(a, b=None, pairs=None, collapse: bool = False) -> EditDistances:
    """Unit-cost Levenshtein distance between code strings.  a, b: `codes.UtteranceCodes` or lists of 1-D int64 device
    tensors; b=None compares `a` with itself; pairs as in dtw().  The symbols are compared, never used as an index.
    collapse=True compares the run-length units of every string (codes.code_runs: frames -> units) instead of its
    frames - that reads the unit counts back once.  -> `EditDistances`."""
    rows_a = _symbol_rows(a, "edit_distance(): a")
    rows_b = None if b is None else _symbol_rows(b, "edit_distance(): b")
    pr = default_pairs(len(rows_a), None if rows_b is None else len(rows_b), pairs)
    if collapse:
        ra = _units(rows_a)
        rb = ra if rows_b is None else _units(rows_b)
    else:
        ra = _ragged(rows_a, "edit_distance(): a", torch.int64)
        rb = ra if rows_b is None else _ragged(rows_b, "edit_distance(): b", torch.int64)
    run = _Launches(L.ALIGN_EDIT, 0, ra, rb, pr, False, None).run("edit_distance()")
    la, lb = np.asarray(ra.length, np.int64)[pr[:, 0]], np.asarray(rb.length, np.int64)[pr[:, 1]]
    longest = np.maximum(la, lb)
    denom = _upload(np.maximum(longest, 1).astype(np.float32), run.dev).view(torch.float32)   # (both empty: 0 / 1)
    return EditDistances(run.steps, run.steps.to(torch.float32) / denom, la, lb)


def _pair_run(N: int, k0: int, k1: int) -> np.ndarray:
    """(k1 - k0, 2) int64: the unordered pairs i < j of N items number k0 .. k1 - 1 in row-major order."""
    first = np.arange(N, dtype=np.int64) * (2 * N - np.arange(N, dtype=np.int64) - 1) // 2    # number of pair (i, i + 1)
    k = np.arange(k0, k1, dtype=np.int64)
    i = np.searchsorted(first, k, side="right") - 1
    return np.stack([i, k - first[i] + i + 1], 1)


def distance_matrix(items, metric: str = "euclid", value: str = "mean", max_pairs: int = 1 << 20) -> torch.Tensor:
    """The (N, N) fp32 matrix of DTW distances between all items: `items` a `Ragged` or a list of (n_u, D) float32 device
    tensors as for dtw().  The N (N - 1) / 2 pairs i < j go through dtw()'s op in runs of at most max_pairs pairs (the
    host pair table and its pinned upload stay bounded; the result does not depend on max_pairs) and each run is
    mirrored into both triangles by one index write.  value "mean": cost / steps, "cost": the summed distance - entry
    (i, j) carries the bits dtw(items, pairs=[(i, j)]) gives, +inf for a pair with an empty side and NaN for one that
    is not finite.  The diagonal is 0.  Nothing here synchronises with the host."""
    metric = _metric_of("distance_matrix()", metric)
    if value not in RANKS:
        raise L.AewError(f"distance_matrix(): value must be one of {sorted(RANKS)}, got '{value}'")
    max_pairs = int(max_pairs)
    if max_pairs < 1:
        raise L.AewError(f"distance_matrix(): max_pairs must be positive, got {max_pairs}")
    ra = _ragged(items, "distance_matrix(): items", torch.float32)
    dev, N = ra.flat.device, len(ra)
    if dev.type != "cuda":
        raise L.AewError(f"the alignment runs on the GPU only (tensor on '{dev}'); there is no CPU path")
    out = torch.zeros(N, N, dtype=torch.float32, device=dev)
    P = N * (N - 1) // 2
    for k0 in range(0, P, max_pairs):
        pr = _pair_run(N, k0, min(P, k0 + max_pairs))
        run = _Launches(L.ALIGN_DTW, metric, ra, ra, pr, False, None).run("distance_matrix()")
        v = run.cost / run.steps if value == "mean" else run.cost
        ij = _upload(np.concatenate([pr, pr[:, ::-1]]), dev).view(torch.int64).reshape(-1, 2)
        out[ij[:, 0], ij[:, 1]] = torch.cat([v, v])
    return out


ABX_MODES = {"within": L.ABX_WITHIN, "across": L.ABX_ACROSS, "any": L.ABX_WITHIN}


class AbxTables:
    """What abx_tables() returns, all on the host.  perm (N,) int32: the item at every sorted position; groups: (G,)
    aew_abx_group_t records; partner (C, S) int32: the group of (category index, speaker index) or -1; categories /
    speakers: the labels by index, in order of first appearance; group_of (N,) int64: the group of every sorted
    position; mode and the op's own mode."""

    def __init__(self, perm, groups, partner, categories, speakers, mode):
        self.perm, self.groups, self.partner = perm, groups, partner
        self.categories, self.speakers, self.mode, self.op_mode = categories, speakers, mode, ABX_MODES[mode]
        self.group_of = np.repeat(np.arange(len(groups), dtype=np.int64), groups["hi"] - groups["lo"])

    N, G = property(lambda self: len(self.perm)), property(lambda self: len(self.groups))
    C, S = property(lambda self: len(self.categories)), property(lambda self: len(self.speakers))

    def __iter__(self):
        return iter((self.perm, self.groups, self.partner, self.categories, self.speakers))


def _labels(x, what: str) -> list:
    x = x.tolist() if isinstance(x, (np.ndarray, torch.Tensor)) else list(x)
    for v in x:
        try:
            hash(v)
        except TypeError:
            raise L.AewError(f"abx_tables(): {what} labels must be hashable, got {type(v).__name__}") from None
    return x


def abx_tables(category, speaker=None, mode: str = "within") -> AbxTables:
    """The host tables of AEW_OP_ABX_COUNT from the labels of N items: category / speaker any sequences of N hashable
    labels (integers, strings, ...).  mode "within": A, B and X of one speaker; "across": A and B of one speaker, X of
    another; "any": speaker-blind - every item gets speaker 0 (speaker=None is allowed only here).  The items are sorted
    stably by (speaker index, category index), indices in order of first appearance.  -> `AbxTables`."""
    if mode not in ABX_MODES:
        raise L.AewError(f"abx_tables(): mode must be one of {sorted(ABX_MODES)}, got '{mode}'")
    cat = _labels(category, "category")
    N = len(cat)
    if N < 1:
        raise L.AewError("abx_tables(): at least one item expected")
    if speaker is None:
        if mode != "any":
            raise L.AewError(f"abx_tables(): mode '{mode}' needs speaker labels; only mode 'any' goes without")
        spk = [0] * N
    else:
        spk = _labels(speaker, "speaker")
        if len(spk) != N:
            raise L.AewError(f"abx_tables(): {N} category labels and {len(spk)} speaker labels")
        if mode == "any":
            spk = [0] * N
    cats, spks = list(dict.fromkeys(cat)), list(dict.fromkeys(spk))
    ci_of, si_of = {c: k for k, c in enumerate(cats)}, {s: k for k, s in enumerate(spks)}
    ci, si = np.array([ci_of[c] for c in cat], np.int64), np.array([si_of[s] for s in spk], np.int64)
    perm = np.lexsort((ci, si))                                               # stable: ties keep the items' order
    key = (si * len(cats) + ci)[perm]
    lo = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    groups = np.zeros(len(lo), dtype=L.ABX_GROUP_DTYPE)
    groups["lo"], groups["hi"] = lo, np.concatenate([lo[1:], [N]])
    groups["cat"], groups["spk"] = key[lo] % len(cats), key[lo] // len(cats)
    partner = np.full((len(cats), len(spks)), -1, np.int32)
    partner[groups["cat"], groups["spk"]] = np.arange(len(lo), dtype=np.int32)
    return AbxTables(perm.astype(np.int32), groups, partner, cats, spks, mode)


class AbxResult:
    """What abx_score() returns; every tensor lies where the counts lie (the device).  error: fp64 scalar, the mean of
    by_category over its present ordered pairs (NaN when no cell is valid); pooled: fp64 scalar, all triples in one pool,
    sum wrong2 / (2 sum n); by_category (C, C) fp64: [cX][cB], NaN where no cell is present; cells: (wrong2, n), two
    (G, G) int64 sums [group of X][group of B]; n_triples: int64 scalar; n_nan: int64 scalar, the NaNs off the diagonal
    of the distance matrix (None from abx_aggregate alone); categories / speakers: the labels by index; tables: the
    `AbxTables`; wrong2 / n: the op's (N, G) counts, rows in sorted order (tables.perm)."""

    def __init__(self, error, pooled, by_category, cells, n_triples, tables, wrong2, n, n_nan=None):
        self.error, self.pooled, self.by_category, self.cells, self.n_triples = error, pooled, by_category, cells, n_triples
        self.tables, self.categories, self.speakers = tables, tables.categories, tables.speakers
        self.wrong2, self.n, self.n_nan = wrong2, n, n_nan


def abx_aggregate(wrong2: torch.Tensor, n: torch.Tensor, tables: AbxTables) -> AbxResult:
    """The op's (N, G) counts (any integer dtype, on any device) -> `AbxResult`: pure torch and dense throughout.  An
    index_add of the rows over X's group gives the int64 (G, G) sums; a cell with n > 0 has the error wrong2 / (2 n); the
    mean over the cells present of a category pair gives by_category, the mean over its present pairs the error."""
    dev, G, C = wrong2.device, tables.G, tables.C
    if wrong2.shape != (tables.N, G) or n.shape != (tables.N, G) or n.device != dev:
        raise L.AewError(f"abx_aggregate(): two ({tables.N}, {G}) tensors on one device expected")
    put = (lambda a: _upload(a, dev).view(torch.int64)) if dev.type == "cuda" else torch.from_numpy
    group_of, cat = put(tables.group_of), put(tables.groups["cat"].astype(np.int64))
    W = torch.zeros(G, G, dtype=torch.int64, device=dev).index_add_(0, group_of, wrong2.to(torch.int64))
    Nn = torch.zeros(G, G, dtype=torch.int64, device=dev).index_add_(0, group_of, n.to(torch.int64))
    present = Nn > 0
    err = torch.where(present, W.to(torch.float64) / (2.0 * Nn.clamp(min=1).to(torch.float64)), 0.0)
    pair = (cat[:, None] * C + cat[None, :]).reshape(-1)
    total = torch.zeros(C * C, dtype=torch.float64, device=dev).index_add_(0, pair, err.reshape(-1))
    count = torch.zeros(C * C, dtype=torch.float64, device=dev).index_add_(0, pair, present.reshape(-1).to(torch.float64))
    by_category = (total / count).reshape(C, C)                               # 0 / 0: NaN where nothing is present
    have = count > 0
    error = torch.where(have, total / count.clamp(min=1.0), 0.0).sum() / have.sum().to(torch.float64)
    n_triples = Nn.sum()
    pooled = W.sum().to(torch.float64) / (2.0 * n_triples.to(torch.float64))
    return AbxResult(error, pooled, by_category, (W, Nn), n_triples, tables, wrong2, n)


def abx_score(dist: torch.Tensor, category, speaker=None, mode: str = "within") -> AbxResult:
    """ABX discriminability of N labelled items from their (N, N) fp32 device matrix of distances (row X, column A or B;
    no symmetry is assumed): for every X, every A of X's category and every B of another one - A and B of one speaker,
    which is X's ("within") or another ("across"); "any" ignores speakers - the triple is wrong when
    dist[X, A] > dist[X, B] and half wrong when neither is smaller (a tie or a NaN).  AEW_OP_ABX_COUNT counts on the
    device, abx_aggregate() averages (see the module text for the rule).  A row pitch is passed on (dist[:, :N] of a
    wider matrix is read in place); any other layout is refused.  N <= 16384.  Nothing here synchronises with the
    host.  -> `AbxResult`."""
    if not torch.is_tensor(dist) or dist.dim() != 2 or dist.shape[0] != dist.shape[1] or dist.dtype != torch.float32:
        raise L.AewError("abx_score(): an (N, N) float32 tensor expected")
    dev, N = dist.device, int(dist.shape[0])
    if dev.type != "cuda":
        raise L.AewError(f"abx_score() runs on the GPU only (tensor on '{dev}'); there is no CPU path")
    ld = int(dist.stride(0)) if N > 1 else max(int(dist.stride(0)), 1)
    if N < 1 or (N > 1 and (dist.stride(1) != 1 or ld < N)):
        raise L.AewError(f"abx_score(): rows of unit stride and a pitch >= N expected, got strides {tuple(dist.stride())}")
    tb = abx_tables(category, speaker, mode)
    if tb.N != N:
        raise L.AewError(f"abx_score(): {tb.N} labels for a matrix of {N} items")
    partner = np.ascontiguousarray(tb.partner)
    d_perm, d_groups, d_partner = (_upload(t, dev) for t in (tb.perm, tb.groups, partner))
    n = torch.empty(N, tb.G, dtype=torch.int32, device=dev)                   # (uint32 words; no count reaches 2^31)
    wrong2 = torch.empty(N, tb.G, dtype=torch.int32, device=dev)
    r = L.AbxCount()
    r.mode, r.N, r.G, r.C, r.S, r.ld = tb.op_mode, N, tb.G, tb.C, tb.S, ld
    r.dist = dist.data_ptr()
    r.perm, r.perm_host = d_perm.data_ptr(), tb.perm.ctypes.data
    r.groups, r.groups_host = d_groups.data_ptr(), tb.groups.ctypes.data
    r.partner, r.partner_host = d_partner.data_ptr(), partner.ctypes.data
    r.n, r.wrong2 = n.data_ptr(), wrong2.data_ptr()
    _run_records(dev, L.OP_ABX_COUNT, "abx", [r], "abx_score()")
    res = abx_aggregate(wrong2, n, tb)
    nan = torch.isnan(dist)
    res.n_nan = nan.sum() - nan.diagonal().sum()
    return res


def abx_task(items, category, speaker=None, mode: str = "within", metric: str = "euclid", value: str = "mean",
             max_pairs: int = 1 << 20) -> AbxResult:
    """abx_score(distance_matrix(items, metric, value, max_pairs), category, speaker, mode): the ABX discriminability of
    labelled sequences under DTW, from the features to the score without a host wait."""
    return abx_score(distance_matrix(items, metric=metric, value=value, max_pairs=max_pairs), category, speaker, mode)


def abx(d_ax: torch.Tensor, d_bx: torch.Tensor) -> torch.Tensor:
    """The ABX error of paired distances: X belongs with A, so a triple is wrong when d(A, X) > d(B, X) and counts one
    half when the two are equal - the fraction with d_ax >= d_bx, ties halved, as a device scalar."""
    if d_ax.shape != d_bx.shape or d_ax.dim() != 1 or d_ax.numel() < 1:
        raise L.AewError(f"abx(): two (P,) tensors expected, got {tuple(d_ax.shape)} and {tuple(d_bx.shape)}")
    if d_ax.device != d_bx.device:
        raise L.AewError("abx(): the two tensors lie on different devices")
    return ((d_ax > d_bx).to(torch.float32) + 0.5 * (d_ax == d_bx).to(torch.float32)).mean()
