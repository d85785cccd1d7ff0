"""Gradient noise analysis on the device: the reference's `grad_analysis.py` (mu_s_incr, quantiles, grad_stats) - "whether
the batch size is too small and thus too noisy for a given learning rate" - as two ops over the flat parameter-sized
buffers (include/aewavenet.h):

  AEW_OP_GRAD_WELFORD  one launch per gradient sample folds it into a running mean `mu` and sum of squared deviations `s`
                       (the reference: six elementwise kernels per tensor and batch)
  AEW_OP_SEG_SELECT    every quantile of every tensor in one op, an exact k-th smallest by radix select (the reference: one
                       kthvalue and one .item() per tensor and quantile)

    import grad_analysis                       # resolves to this file when ae-wavenet_amd/ is first on sys.path
    q = grad_analysis.grad_stats(model, closure, n_batch, [0, .1, .25, .5, .75, .9, 1])      # the reference's call

    gs = grad_analysis.GradStats(model)        # the streaming form, in a training loop
    loss.backward(); gs.add()                  # device only, no host synchronisation
    gs.sigma_quantiles([.5, .9]); gs.noise_scale(batch_size)

No CPU path: the HIP library is required.
"""
from __future__ import annotations

import ctypes as C

import torch

try:
    from . import _lib as L
    from .plan import Plan
except ImportError:                                     # imported as the top-level module `grad_analysis`
    from ae_wavenet_amd import _lib as L
    from ae_wavenet_amd.plan import Plan


def ranks(qs, numel: int):
    """The reference's rank of quantile q in a tensor of `numel` elements (grad_analysis.py:48): 1-based, Python's round
    (half to even), on the host."""
    return [1 + round(float(q) * (numel - 1)) for q in qs]


class GradStats:
    """Running per-weight mean and sum of squared deviations of the gradient, and what is read off them.

    add() goes after `loss.backward()`: ONE launch over the flat gradient buffer, no host synchronisation, with the
    engine's plans captured or not.  It writes nothing a training step reads: parameters, gradients, optimizer moments,
    average and counters keep their bits.  `mu` / `s` are two flat fp32 buffers by the ParamStore offset rule
    (FusedAdam._layout) that belong to this object: allocated at the first add(), they survive an engine rebuild for
    another batch size - add() reads the gradient buffer of whichever engine is live.

    reference_counts=False: sample b (0-based) is folded with divisor b + 1, the formula the reference's header quotes.
    True: divisor b, what the reference's grad_stats passes (its loop index): sample 0 is overwritten at b = 1, and at
    b = 1 mu' can overshoot the sample, so s may come out slightly negative (its sigma is then NaN, as the reference's).

    names: restrict the statistics to these parameters (named_parameters() order is kept); a model without an engine
    (any nn.Module on the device) or a restricted set has its .grad tensors packed into a flat buffer of this object's
    first (device copies).

    Data parallel: under the all-reduce schedule add() folds what .grad shows - the reduced gradient, identical on every
    rank.  Under the sharded schedule a rank holds the reduced gradient of its own shards only: add() raises."""

    def __init__(self, model, reference_counts: bool = False, names=None):
        self.model = model
        self.reference_counts = bool(reference_counts)
        self._names = None if names is None else list(names)
        self.count = 0                                   # samples folded
        self.mu = self.s = None
        self._lay = None

    # ---- layout ------------------------------------------------------------------------------------------------------
    def _layout(self):
        if self._lay is None:
            named = list(self.model.named_parameters())
            if self._names is not None:
                want = set(self._names)
                named = [(n, p) for n, p in named if n in want]
            lay, o = [], 0
            for n, p in named:
                lay.append((n, o, p.numel(), tuple(p.shape)))
                o += (p.numel() + 3) // 4 * 4
            if not lay:
                raise L.AewError("GradStats: no parameter takes part")
            self._lay, self.numel = lay, o
            self._whole = self._names is None or len(lay) == len(list(self.model.named_parameters()))
        return self._lay

    @property
    def names(self):
        return [n for n, _, _, _ in self._layout()]

    def _alloc(self, device):
        lay = self._layout()
        P, n = len(lay), self.numel
        self.device = device
        # (+64 elements of slack, like the engine's workspace buffers)
        self.mu = torch.zeros(n + 64, dtype=torch.float32, device=device)
        self.s = torch.zeros(n + 64, dtype=torch.float32, device=device)
        self._gbuf = None
        chunks, first = L.uw_chunks([o for _, o, _, _ in lay], [k for _, _, k, _ in lay])
        nch = first[-1]
        self._chunks_host, self._first_host, self.n_chunks = chunks, first, nch
        self._chunks = torch.frombuffer(bytearray(bytes(chunks))[:16 * nch], dtype=torch.int64).to(device)
        self._first = torch.tensor(first, dtype=torch.int32, device=device)
        self._part = torch.zeros(2 * nch + 2, dtype=torch.float64, device=device)
        self._sums = torch.zeros(2 * P, dtype=torch.float64, device=device)
        self._part_live = False
        w = L.GradWelford()
        w.mu, w.s, w.n = self.mu.data_ptr(), self.s.data_ptr(), n
        w.chunks, w.chunks_host, w.n_chunks = self._chunks.data_ptr(), C.addressof(chunks), nch
        w.part = self._part.data_ptr()
        self._wel = Plan("grad welford")
        self._wel.add(L.OP_GRAD_WELFORD, w, "grad welford")
        r = L.UpdateRatio()
        r.part, r.first, r.n_tensors, r.finalize = self._part.data_ptr(), self._first.data_ptr(), P, 0
        r.sums = self._sums.data_ptr()
        self._red = Plan("grad stats sums")
        self._red.add(L.OP_UPDATE_RATIO, r, "grad stats sums")
        self._sel, self._sel_key, self._rank_tabs = None, None, {}

    def _stream(self) -> int:
        if self.device.type != "cuda":
            raise L.AewError("GradStats runs only through the HIP library on an MI355X")
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---- the gradient sample -----------------------------------------------------------------------------------------
    def _sample(self) -> torch.Tensor:
        """The flat gradient sample: the live engine's gradient buffer, or this object's packed copy of the .grad tensors."""
        lay = self._layout()
        eng = getattr(self.model, "_engine", None)
        if eng is not None and self._whole:
            if eng.ps.numel != self.numel:
                raise L.AewError("GradStats: the engine's flat layout is not the model's")
            return eng.ps.grads
        params = dict(self.model.named_parameters())
        g0 = params[lay[0][0]].grad
        if g0 is None:
            raise L.AewError(f"GradStats.add(): parameter {lay[0][0]} has no gradient")
        if self.mu is None:
            self._alloc(g0.device)
        if self._gbuf is None:
            self._gbuf = torch.zeros(self.numel + 64, dtype=torch.float32, device=self.device)
        for n, o, k, _ in lay:
            g = params[n].grad
            if g is None:
                raise L.AewError(f"GradStats.add(): parameter {n} has no gradient")
            self._gbuf[o:o + k].copy_(g.detach().reshape(-1))
        return self._gbuf

    def add(self):
        """Fold the gradients of the last backward in (AEW_OP_GRAD_WELFORD; the chunk sums sums() / noise_scale() read come
        out of the same launch)."""
        if getattr(getattr(self.model, "_schedule", None), "shards", False):      # (any nn.Module: no schedule, no shards)
            raise L.AewError("GradStats.add() is not supported under the sharded data-parallel schedule: each rank holds the "
                             "reduced gradient of its own shards only")
        with torch.no_grad():
            g = self._sample()
            if self.mu is None:
                self._alloc(g.device)
            b = self.count
            w = self._wel.array()[0].u.gwel
            w.g, w.first = g.data_ptr(), int(b == 0)
            w.divisor = float(b if self.reference_counts else b + 1)
            with torch.cuda.device(self.device):
                self._wel.run(self._stream())
            self.count = b + 1
            self._part_live = True

    def reset(self):
        """Forget every sample (the buffers stay)."""
        self.count = 0
        self._part_live = False
        if self.mu is not None:
            self.mu.zero_()
            self.s.zero_()
            self._part.zero_()

    # ---- what is read off the statistics -----------------------------------------------------------------------------
    def _need(self):
        if self.mu is None or self.count < 1:
            raise L.AewError("GradStats: no sample folded yet (add() after a backward)")

    def view(self, name: str, which: str) -> torch.Tensor:
        """A view of one tensor's statistics: which = "mu" (running mean) or "s" (running sum of squared deviations)."""
        self._need()
        if which not in ("mu", "s"):
            raise ValueError(f"Invalid statistic: {which!r} ('mu' or 's')")
        for n, o, k, shp in self._layout():
            if n == name:
                return (self.mu if which == "mu" else self.s)[o:o + k].view(shp)
        raise KeyError(name)

    def select(self, k: torch.Tensor, denom: float = 1.0, raw: bool = False) -> torch.Tensor:
        """AEW_OP_SEG_SELECT over `s`: k int32 [P][Q] device table of 1-based ranks -> float32 [P][Q], the k-th smallest s of
        every tensor as sqrt(s / denom), or s itself with raw.  No host synchronisation."""
        self._need()
        P = len(self._layout())
        if k.dtype != torch.int32 or k.dim() != 2 or k.shape[0] != P or not 1 <= k.shape[1] <= L.SELECT_MAX_Q \
                or k.device != self.mu.device or not k.is_contiguous():
            raise ValueError(f"ranks: a contiguous int32 [{P}][1..{L.SELECT_MAX_Q}] tensor on {self.mu.device}")
        Q = k.shape[1]
        if self._sel_key != Q:
            p = L.SegSelect()
            p.s, p.chunks, p.n_chunks, p.n_tensors, p.Q = self.s.data_ptr(), self._chunks.data_ptr(), self.n_chunks, P, Q
            nbytes = C.c_int64()
            L.check(L.load().aew_seg_select_size(C.byref(p), C.byref(nbytes)), "aew_seg_select_size")
            self._scratch = torch.zeros(nbytes.value // 4 + 4, dtype=torch.int32, device=self.device)
            p.scratch = self._scratch.data_ptr()
            self._sel = Plan("grad stats select")
            self._sel.add(L.OP_SEG_SELECT, p, "seg select")
            self._sel_key = Q
        out = torch.empty(P, Q, dtype=torch.float32, device=self.device)
        p = self._sel.array()[0].u.ssel
        p.k, p.out, p.denom, p.raw = k.data_ptr(), out.data_ptr(), float(denom), int(bool(raw))
        with torch.cuda.device(self.device):
            self._sel.run(self._stream())
        return out

    def rank_table(self, qs) -> torch.Tensor:
        """int32 [P][Q] on the device: ranks(qs, numel) of every tensor (a host table, uploaded without a synchronisation)."""
        qs = tuple(float(q) for q in qs)
        if not qs:
            raise ValueError("at least one quantile")
        tab = self._rank_tabs.get(qs)
        if tab is None:
            tab = torch.tensor([ranks(qs, k) if k > 0 else [1] * len(qs) for _, _, k, _ in self._layout()], dtype=torch.int32)
            tab = self._rank_tabs[qs] = tab.to(self.mu.device, non_blocking=True)
        return tab

    def sigma_quantiles(self, qs, denom=None) -> torch.Tensor:
        """float32 [P][Q] device tensor, named_parameters() order: quantile q of the per-weight standard deviation
        sqrt(s / denom) of every tensor, the k-th smallest with the reference's rank rule (ranks()).  denom defaults to the
        number of samples folded.  More than 8 quantiles take one op per 8."""
        self._need()
        qs = list(qs)
        denom = float(self.count if denom is None else denom)
        outs = [self.select(self.rank_table(qs[i:i + L.SELECT_MAX_Q]), denom) for i in range(0, len(qs), L.SELECT_MAX_Q)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, 1)

    def sums(self) -> torch.Tensor:
        """float64 [2][P] on the device: sum of s and sum of mu^2 per tensor - the chunk sums of the last add() reduced by
        AEW_OP_UPDATE_RATIO (finalize = 0), one fixed order."""
        self._need()
        with torch.cuda.device(self.device):
            self._red.run(self._stream())
        return self._sums.view(2, -1).clone()

    def noise_scale(self, batch_size) -> torch.Tensor:
        """The simple noise scale in samples, a 0-d float64 device tensor: batch_size * tr / (sum mu^2 - tr / count) with
        tr = sum s / (count - 1) over all tensors - the trace of the per-weight gradient covariance at this batch size
        over the squared norm of the mean gradient, corrected for the noise in that mean.  NaN for count < 2."""
        self._need()
        if self.count < 2:
            return torch.full((), float("nan"), dtype=torch.float64, device=self.device)
        t = self.sums().sum(1)
        tr = t[0] / (self.count - 1)
        return float(batch_size) * tr / (t[1] - tr / self.count)


def grad_stats(model, update_model_closure, n_batch, report_quantiles, *, reference_counts=True):
    """Drop-in for the reference's grad_stats (grad_analysis.py:53-85), same signature and call pattern: one closure call
    whose gradients only decide which parameters take part (those whose .grad is None are left out), then n_batch calls,
    each folded into running statistics on the device; returns {parameter name: [quantile of the per-weight standard
    deviation sqrt(s / n_batch), ...]} as Python floats - ONE device-to-host copy of the [P][Q] table at the end and no
    other synchronisation.

    reference_counts=True (the default) reproduces the reference bit for bit, including what its counting does: it passes
    the loop index b as the count, so sample 0 is overwritten at b = 1 and n_batch - 1 samples are normalised by n_batch;
    at b = 1 the new mean can overshoot the sample and s goes slightly negative for some weights, whose sigma is NaN and
    ranks last, as in the reference.  reference_counts=False folds sample b with divisor b + 1, the formula the
    reference's header quotes."""
    update_model_closure()
    names = [name for name, par in model.named_parameters() if par.grad is not None]
    gs = GradStats(model, reference_counts=reference_counts, names=names)
    for _ in range(n_batch):
        update_model_closure()
        gs.add()
    qs = list(report_quantiles)
    if gs.count < 1 or not qs:
        return {name: [] for name in names}
    table = gs.sigma_quantiles(qs, denom=n_batch).cpu()
    return {name: [float(v) for v in table[i]] for i, name in enumerate(gs.names)}
