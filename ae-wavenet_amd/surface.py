"""Shared machinery of the drop-in nn.Module surfaces (see autoencoder_model.py and
mfcc_inverter.py in this package).

The reference harness drives a model through (chassis.py:151-171, checkpoint.py:35-67):
    model = Model(hps); model.get_input_size(w); model.override(w); model.mfcc
    optim = Adam(model.parameters()); model.to(device); model.train()
    quant, target, loss = model.run(wav, mel, voice, jitter); loss.backward(); optim.step()
    model.objective.metrics, model.encoder.metrics, model.bn_type,
    model.bottleneck.update_codebook(), model.init_codebook(...)

Parameters are nn.Parameters whose storage is a view into the engine's flat fp32 buffer and
whose .grad is a view into the flat gradient buffer, so `loss.backward()` (one
autograd.Function around the whole HIP training step) fills every .grad without per-parameter
autograd traffic, and any torch optimizer — or the fused `optim.FusedAdam` — can step them.
"""
from __future__ import annotations

import contextlib
import math
import operator
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import geometry as G
from .dp import LocalSchedule
from .model import OptState, TrainEngine


_RESTART_DEFAULTS = dict(max_codes=64, denom_init=1.0, seed=0)


def _check_codebook_restart(opt):
    """The `codebook_restart` constructor option: None, or dict(every=int >= 1, min_usage=float > 0, max_codes=64,
    denom_init=1.0, seed=0) -> a complete dictionary of plain Python numbers."""
    if opt is None:
        return None
    if not isinstance(opt, dict):
        raise ValueError(f"Invalid codebook_restart: {opt!r} (None, or a dict with every, min_usage and optionally "
                         "max_codes, denom_init, seed)")
    unknown = set(opt) - {"every", "min_usage"} - set(_RESTART_DEFAULTS)
    if unknown or "every" not in opt or "min_usage" not in opt:
        raise ValueError(f"Invalid codebook_restart: {opt!r} (keys every and min_usage, optionally max_codes, denom_init, "
                         "seed)")
    out = dict(_RESTART_DEFAULTS, **opt)

    def whole(name, lo, hi):
        v = out[name]
        try:                                                     # Python and numpy integers; no bool, no float
            i = None if isinstance(v, bool) else operator.index(v)
        except TypeError:
            i = None
        if i is None or not lo <= i <= hi:
            raise ValueError(f"Invalid codebook_restart[{name!r}]: {v!r} (an integer in {lo} .. {hi})")
        out[name] = i

    def positive(name):
        try:                                                     # whatever float() takes, like FusedAdam's options
            f = float(out[name])
        except (TypeError, ValueError):
            f = float("nan")
        if isinstance(out[name], bool) or not (math.isfinite(f) and f > 0.0):
            raise ValueError(f"Invalid codebook_restart[{name!r}]: {out[name]!r} (a finite number > 0)")
        out[name] = f

    whole("every", 1, 2 ** 62)
    whole("max_codes", 1, L.VQ_RESTART_MAX)
    whole("seed", 0, 2 ** 64 - 1)
    positive("min_usage")
    positive("denom_init")
    return out


def _check_accumulate(k):
    """The `accumulate` option: a whole number >= 1 (Python and numpy integers; no bool, no fraction, no string)."""
    try:
        i = None if isinstance(k, bool) else operator.index(k)
    except TypeError:
        i = None
    if i is None or not 1 <= i <= 2 ** 31 - 1:
        raise ValueError(f"Invalid accumulate: {k!r} (micro-batches per optimizer step: an integer >= 1)")
    return i


class _StepFn(torch.autograd.Function):
    """loss = f(parameters, batch) with a hand-written backward (the bwd plan)."""

    @staticmethod
    def forward(ctx, anchor, owner):
        ctx.owner = owner
        ctx.fold = fold = owner._begin_micro_step()          # None without accumulation; else (mode, micro-step)
        loss = owner._schedule.forward(owner._engine, owner._ema_allreduce, None if fold is None else fold[0])
        ctx.act = (owner._engine.serial, owner._engine.act_epoch)    # whose activations, and which, the backward reads
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        # g = d(L)/d(loss) from autograd ((loss * k).backward(), loss scaling, ...).  It is copied device-side into
        # the engine's `gmul` scalar, which the ops where the loss gradient enters the backward plan multiply in, so
        # every .grad carries it.  The backward plan WRITES the flat gradient buffer; nn.Module semantics (a second
        # backward() without zero_grad() adds to .grad) are kept by carrying the previous values over explicitly - a
        # path the reference harness never takes (it zeroes every step, chassis.py:157-160; FusedAdam.zero_grad() /
        # zero_grad(set_to_none=True) cost nothing here).
        owner = ctx.owner
        eng = owner._engine
        if eng is None or (eng.serial, eng.act_epoch) != ctx.act:
            raise L.AewError("loss.backward() after model.evaluate() / encode() / decode(): that call overwrote the activations "
                             "(and code indices, logits) this loss was computed from, so its gradients would be those of another "
                             "batch.  Call backward() first, or run() the batch again.  No gradient was written")
        eng.set_upstream_grad(g)
        mode, j = ctx.fold or (None, 0)
        if mode is None:
            prev = owner._grads_carried()
        else:                                                # accumulate > 1: the accumulator carries the group
            if j != owner._micro:
                raise L.AewError(f"loss.backward() out of order: this loss belongs to micro-step {j + 1} of the accumulated "
                                 f"group, the group stands at micro-step {owner._micro + 1} (one backward() per run(), in "
                                 "order; model.reset_accumulation() discards the open group).  No gradient was written")
            prev, owner._grads_cleared = None, False
        # collectives, the codebook upkeep and the restart belong to the group: they run with its last micro-step only
        last = mode in (None, L.ACCUM_LAST)
        owner._schedule.backward(eng, mode)
        if last:
            owner._auto_restart()                            # (the deferred EMA and the codebook refresh are done by here)
        owner._after_backward(g, reduce=last)
        if mode is not None:
            owner._micro, owner._group_ready = (0 if last else j + 1), last
        if prev is not None:
            eng.ps.grads[:eng.ps.numel].add_(prev)
        # (the anchor's "gradient": a cached zero, not a fill kernel per step)
        z = getattr(owner, "_anchor_zero", None)
        if z is None or z.device != owner._anchor.device:
            z = owner._anchor_zero = torch.zeros_like(owner._anchor)
        return z, None


class Evaluator:
    """What `model.evaluation()` yields: the running record of the model.evaluate() calls made inside the block."""

    def __init__(self, model, group=None):
        self._model = model
        self._group = group                # a grouping block: ("voice" | "group", G)
        self._started = False              # ... whose grouped record an evaluate() of the block has started

    def result(self) -> Dict[str, torch.Tensor]:
        """The record so far as 0-d device tensors (one finalize launch, no host synchronisation; reading a value is the
        caller's): loss (mean per batch), nll (nats per position), bits_per_sample, top1, tprb (mean target probability),
        dist, code_entropy (bits), code_perplexity, codes_used, term1 .. term4 (the loss's terms, mean per batch),
        positions, batches.  The codebook entries are zero for models without a codebook.  Under data parallel the ranks'
        records are summed first (ONE all-reduce; COLLECTIVE: every rank calls it, every rank gets the same values).  More
        evaluate() calls may follow; each result() covers everything since the block was entered."""
        m = self._model
        eng = m._engine
        if eng is None:
            raise L.AewError("Evaluator.result(): no engine - nothing has been evaluated on this device yet")
        with torch.no_grad():
            out = m._schedule.eval_finish(eng).clone()
        return {name: out[i] for i, name in enumerate(L.EVAL_OUT_NAMES)}

    def _grouped_engine(self, what: str):
        eng = self._model._engine
        if self._group is None:
            raise L.AewError(f"Evaluator.{what}: this block does not group - use model.evaluation(by='voice') or "
                             "model.evaluation(groups=G)")
        if eng is None or eng.eval_gfin is None or not self._started:
            raise L.AewError(f"Evaluator.{what}: nothing has been evaluated inside this block yet")
        return eng

    def by_group(self) -> Dict[str, torch.Tensor]:
        """The record so far, split over the groups: a dict of (G,) float32 device tensors - windows, positions, nll
        (nats per position), bits_per_sample, top1, tprb, dist, queries, code_entropy (bits, of the group's own code
        distribution), code_perplexity, codes_used.  A group that saw no window reads 0 throughout.  One finalize
        launch, no host synchronisation; under data parallel the ranks' grouped records are summed first (ONE
        all-reduce; COLLECTIVE).  Without a codebook the three code entries are 0.  Counts above 2^24 are rounded by
        fp32; counts() has the exact table."""
        eng = self._grouped_engine("by_group()")
        with torch.no_grad():
            gout, _ = self._model._schedule.eval_group_finish(eng)
        return {name: gout[:, i] for i, name in enumerate(L.EVAL_GOUT_NAMES)}

    def information(self) -> Dict[str, torch.Tensor]:
        """What the codes tell about the group, from the (group, code) table of the record so far, as 0-d float32
        device tensors (entropies in bits): n (counted queries), code_entropy H(C), group_entropy H(G), cond_entropy
        H(C|G), mutual_information I(C;G), mutual_information_mm (Miller-Madow corrected: I - (cells - groups_used -
        codes_used + 1) / (2 n ln 2); NOT clamped, slightly negative values occur when the codes are independent of the
        group), mi_over_group_entropy, mi_over_code_entropy, cells (non-zero table entries), groups_used, codes_used,
        dropped_windows (group id outside [0, G)), batches.  The plug-in value I overestimates when the queries are few
        against G * K cells; the corrected value is the one to compare across runs then.  One finalize launch, no host
        synchronisation; ONE all-reduce under data parallel (COLLECTIVE).  fp32 rounds counts above 2^24: counts()
        is exact.  Raises AewError for a model without discrete codes."""
        self._model._need_codes("Evaluator.information()")
        eng = self._grouped_engine("information()")
        with torch.no_grad():
            _, tout = self._model._schedule.eval_group_finish(eng)
        return {name: tout[i] for i, name in enumerate(L.EVAL_TOUT_NAMES)}

    def counts(self) -> torch.Tensor:
        """A (G, K) int64 copy of THIS rank's (group, code) table: the exact counts (the fp32 outputs of by_group() /
        information() round above 2^24).  No collective, no host synchronisation."""
        self._model._need_codes("Evaluator.counts()")
        eng = self._grouped_engine("counts()")
        return eng.eval_ghist.to(torch.int64) & 0xffffffff

    def windows(self) -> Dict[str, torch.Tensor]:
        """Per-window means of the LAST evaluated batch, as (B,) float32 device tensors: nll (nats per position), top1,
        tprb, dist (0 without a codebook) - per-utterance scoring without a second pass.  Also filled for a window
        whose group id was dropped.  No launch of the library, no host synchronisation."""
        eng = self._grouped_engine("windows()")
        win = eng.eval_win
        n_pos = float(eng.n_win - 1)
        out = {"nll": win[:, 0] / n_pos, "top1": win[:, 2] / n_pos, "tprb": win[:, 1] / n_pos}
        out["dist"] = win[:, 3] / float(eng.Q // eng.B) if eng.eval_ghist is not None else torch.zeros_like(win[:, 3])
        return {k: v.to(torch.float32) for k, v in out.items()}


class Objective:
    """Stand-in for the reference loss modules' attribute surface (metrics dict,
    update_anneal_weight, free_nats, anneal_weight; chassis.py:124,149,215-220)."""

    def __init__(self, owner):
        self._owner = owner
        self.metrics: Dict[str, torch.Tensor] = {}
        self.free_nats = torch.tensor(float(getattr(owner.hps, "bn_free_nats", 0.0)))
        self.anneal_weight = torch.tensor(0.0)

    def update_anneal_weight(self, w):
        self.anneal_weight = torch.tensor(float(w))
        eng = self._owner._engine
        if eng is not None and eng.bn_type == "vae":
            eng.set_anneal_weight(float(w))


class _EncoderFacade(nn.Module):
    def __init__(self):
        super().__init__()
        self.metrics: Dict[str, torch.Tensor] = {}


class _BottleneckFacade(nn.Module):
    def __init__(self, owner):
        super().__init__()
        self.__dict__["_owner"] = owner

    def update_codebook(self):
        """vqema_bn.py:216-222 (called by chassis.py:175-176)."""
        eng = self._owner._engine
        if eng is not None and eng.bn_type == "vqvae-ema":
            eng.update_codebook()

    def _restart_engine(self):
        owner = self._owner
        if owner.bn_type != "vqvae-ema":
            raise L.AewError(f"restarting codes needs the vqvae-ema bottleneck (this model: {owner.bn_type}): only its "
                             "codebook carries a usage statistic")
        if owner._engine is None:
            raise L.AewError("no engine yet: restarting codes takes rows of the last run()'s encoder outputs")
        return owner._engine

    def restart_dead_codes(self, min_usage=None, call=None):
        """Re-seed the codes whose EMA count is under `min_usage` from distinct encoder outputs of the last run(), on the
        device (TrainEngine.restart_codes; under data parallel every rank ends up with rank 0's codebook).  min_usage and
        the other settings default to the model's `codebook_restart` option, `call` - the counter the choice of rows is
        hashed from - to the engine's step count.  max_codes, denom_init and seed come from that option alone: a model
        built without it restarts with max_codes=64, denom_init=1.0, seed=0 (TrainEngine.restart_codes takes them
        directly).  Counts: `restart_counts`."""
        owner, eng = self._owner, self._restart_engine()
        opt = owner._restart
        if min_usage is None:
            if opt is None:
                raise L.AewError("restart_dead_codes() needs a threshold: pass min_usage, or build the model with "
                                 "codebook_restart=dict(every=..., min_usage=...)")
            min_usage = opt["min_usage"]
        owner._restart_codes(eng, float(min_usage), eng.step_count if call is None else int(call))

    @property
    def restart_counts(self) -> torch.Tensor:
        """int32 [4] on the device: dead codes found and codes restarted by the last restart, codes restarted so far on
        this engine, 0.  Reading it synchronises."""
        return self._restart_engine().restart_out()


class HipModelBase(nn.Module):
    """Common implementation; subclasses set `kind` and the parameter prefix layout."""

    def __init__(self, hps, kind: str, loss_mode: str = "intended", take_compat: bool = False,
                 update_codebook_every_step: bool = True, n_mel: Optional[int] = None, codebook_restart=None, accumulate=1):
        super().__init__()
        codebook_restart = _check_codebook_restart(codebook_restart)
        accumulate = _check_accumulate(accumulate)
        if hps.global_model != kind:
            hps = type(hps)(hps)
            hps["global_model"] = kind
        self.hps = hps
        self.kind = kind
        self.bn_type = hps.bn_type if kind == "autoencoder" else "none"
        self._opts = dict(loss_mode=loss_mode, take_compat=take_compat,
                          update_codebook_every_step=update_codebook_every_step, n_mel=n_mel)
        if codebook_restart is not None and self.bn_type != "vqvae-ema":
            raise ValueError(f"codebook_restart needs the vqvae-ema bottleneck (this model: {self.bn_type}): only its "
                             "codebook carries a usage statistic")
        self._restart = codebook_restart                 # kept on the model: every engine it builds restarts by it
        self.window_batch_size = hps.n_win_batch
        self._engine: Optional[TrainEngine] = None
        self._engines: Dict[int, TrainEngine] = {}      # engines by batch size (train B, sampling B = 1, ...)
        self._opt_carry: Optional[OptState] = None       # the optimizer state while no engine holds it
        self._grads_cleared = True                       # no backward yet / FusedAdam.zero_grad() since the last one
        self._accumulate = accumulate                    # micro-batches per optimizer step (1: no accumulation)
        self._micro = 0                                  # micro-batches folded into the open group, 0 .. accumulate - 1
        self._group_ready = False                        # .grad holds a whole group's sum that no step() has consumed
        self._fold_open = False                          # a run() of a group has folded its statistics, its backward is due
        self._weights_epoch = 0                          # bumped whenever parameter values change behind torch's back
        self._device = torch.device("cpu")
        self._pending_state: Optional[Dict[str, torch.Tensor]] = None
        self._ema_allreduce = None
        self._dp = None
        self._eval_ev = None                             # inside a grouping evaluation() block: its Evaluator
        self.objective = Objective(self)
        # inference surface (chassis.py:296, 313: model.wavenet.set_n_replicas / .n_quant; `model.wavenet` of the
        # MFCC inverter is the model itself here)
        self.n_quant, self.n_replicas = hps.n_quant, 1
        self.sample_seed = 0
        self.draw = None                                 # default draw controls of the sampling calls (sampler.Draw; None: off)
        self._sampler = None
        self._utt_mfcc = None                            # encode_wavs() / encode_corpus(): the whole-utterance front-end
        self._anchor = torch.zeros((), requires_grad=True)
        # geometry attributes of the reference classes (autoencoder_model.py:119-146,
        # mfcc_inverter.py:38-65)
        self._set_geometry(self.window_batch_size)
        # Parameters exist from construction (Checkpoint builds Adam before .to(device),
        # checkpoint.py:48-50); they are re-homed into the engine's flat buffer on first use.
        self._make_cpu_params()

    def set_n_replicas(self, n_replicas):                       # wavenet.py:296-297
        self.n_replicas = int(n_replicas)

    # ---- geometry / harness queries ------------------------------------------------------
    def _set_geometry(self, w):
        g = G.model_geometry(self.hps, self.kind == "autoencoder", w)
        self.geom = g
        self.enc_in_len, self.enc_in_mel_len, self.embed_len = g.enc_in_len, g.mel_len, g.embed_len
        self.dec_in_len = g.dec_in_len
        self.trim_dec_in = torch.tensor(g.trim_dec_in)
        self.trim_dec_out = torch.tensor(g.trim_dec_out)
        self.trim_ups_out = torch.tensor(g.trim_ups_out)

    def get_input_size(self, output_size):
        """wav samples per window (wavenet.py:287-294 via checkpoint.py:40)."""
        return G.input_size(self.hps, self.kind == "autoencoder", output_size)

    # ---- gradient accumulation: k micro-batches per optimizer step ----------------------------
    @property
    def accumulate(self) -> int:
        """Micro-batches per optimizer step (the constructor's `accumulate`, set_accumulate()).  With k > 1 the k-th
        loss.backward() of a group leaves the SUM of the group's gradients in .grad (the earlier ones leave their own
        micro-batch's), FusedAdam.step() is a no-op until then and applies grad_scale / k - the optimizer sees the MEAN
        of the micro-batch gradients, so do not also divide the loss by k - and the EMA statistics, the codebook
        refresh, the code restart and every data-parallel exchange happen once per group."""
        return self._accumulate

    @property
    def micro_step(self) -> int:
        """Micro-batches folded into the open group so far: 0 .. accumulate - 1."""
        return self._micro

    @property
    def group_ready(self) -> bool:
        """True from the k-th backward of a group until FusedAdam.step() consumes it (or the next group begins)."""
        return self._group_ready

    def set_accumulate(self, k):
        """Change the accumulation count; only between groups."""
        k = _check_accumulate(k)
        if self._micro != 0 or self._group_ready or self._fold_open:
            raise L.AewError("set_accumulate() inside an accumulated group (micro-steps pending, or a finished group no "
                             "step() has consumed): step the optimizer first, or discard the group with "
                             "model.reset_accumulation()")
        self._accumulate = k

    def reset_accumulation(self):
        """Discard the open group: the next run() starts a fresh one.  Nothing is launched; the partial sums are simply
        overwritten by the next group's first micro-step."""
        if self._group_ready:
            self._schedule.abandon()
        self._micro, self._group_ready, self._fold_open = 0, False, False

    def _begin_micro_step(self):
        """The fold of the coming forward / backward pair: None without accumulation, else (AEW_OP_ACCUM mode, micro-step
        index).  Beginning a group while the last one is still unstepped drops that sum, as torch drops an unstepped
        gradient."""
        k = self._accumulate
        if k == 1:
            return None
        if self._group_ready:
            self.reset_accumulation()
        j = self._micro
        if self._fold_open and j > 0:
            raise L.AewError(f"run() at micro-step {j + 1} of {k} while the previous run() of the group has had no "
                             "backward(): its EMA statistics are already folded into the group and would be counted "
                             "twice.  Call loss.backward() after every run() of a group (model.evaluate() computes a "
                             "loss without a training step), or discard the group with model.reset_accumulation()")
        self._fold_open = True
        return (L.ACCUM_LAST if j == k - 1 else L.ACCUM_FIRST if j == 0 else L.ACCUM_ADD), j

    def _refuse_mid_group(self, what):
        """The group's running sums live in the engine: it must not be replaced or dropped before the group is stepped."""
        if self._micro != 0 or self._group_ready:
            raise L.AewError(f"{what} inside an accumulated group (micro-step {self._micro} of {self._accumulate}"
                             f"{', group ready' if self._group_ready else ''}): the engine holds the group's running sums.  "
                             "Step the optimizer first, or discard the group with model.reset_accumulation()")

    def override(self, n_win_batch=None):
        """mfcc_inverter.py:30-35 (checkpoint.py:46)."""
        if n_win_batch is not None and n_win_batch != self.window_batch_size:
            if self._engine is not None:
                self._refuse_while_averaged_in("override()")         # (before anything is changed)
                self._refuse_mid_group("override()")
            self.window_batch_size = n_win_batch
            self._set_geometry(n_win_batch)
            self._drop_engine()

    # ---- parameters --------------------------------------------------------------------------
    def _specs(self):
        from .engine import bottleneck_param_specs, decoder_param_specs, encoder_param_specs
        h = self.hps
        if self.kind == "autoencoder":
            n_mel = self._opts["n_mel"] or 3 * h.n_mfcc
            return (encoder_param_specs(n_mel, h.enc_n_out) + bottleneck_param_specs(h)
                    + decoder_param_specs(h, h.n_lc_in, "decoder."))
        return decoder_param_specs(h, h.n_lc_in, "wavenet.")

    def _make_cpu_params(self):
        """Xavier-uniform weights, zero biases (netmisc.py:10-14); VQ codebooks with the
        reference's gains (vq_bn.py:21)."""
        self._pnames = []
        for name, shape in self._specs():
            t = torch.empty(shape)
            if len(shape) >= 2:
                nn.init.xavier_uniform_(t)
            else:
                t.zero_()
            pname = name.replace(".", "__")
            self.register_parameter(pname, nn.Parameter(t))
            self._pnames.append((name, pname))
        if self.bn_type == "vqvae-ema":
            K, d = self.hps.bn_vq_n_embed, self.hps.bn_n_out
            emb = torch.empty(K, d)
            nn.init.xavier_uniform_(emb, gain=10)                        # vqema_bn.py:97
            comp = 1.0 - self.hps.bn_vq_ema_gamma
            self.register_buffer("bn_emb", emb)
            self.register_buffer("bn_ema_numer", emb * comp)             # vqema_bn.py:117-118
            self.register_buffer("bn_ema_denom", torch.full((K,), comp))
            self.register_buffer("bn_ind_hist", torch.zeros(K))

    # nn.Module hooks so that state_dict / named_parameters use the reference's dotted names
    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        for name, pname in self._pnames:
            yield (prefix + ("." if prefix else "") + name), self._parameters[pname]

    def parameters(self, recurse=True):
        for _, p in self.named_parameters():
            yield p

    _BUF_NAMES = {"bn_emb": "bottleneck.emb", "bn_ema_numer": "bottleneck.ema_numer",
                  "bn_ema_denom": "bottleneck.ema_denom", "bn_ind_hist": "bottleneck.ind_hist"}

    @property
    def _schedule(self):
        """The exchange schedule of a step (dp.LocalSchedule / AllReduceSchedule / ShardedSchedule), asked for at every use:
        tests and tools change the DataParallel's mode, model._dp and model._ema_allreduce after attach()."""
        return LocalSchedule() if self._dp is None else self._dp.schedule()

    def _dp_finish(self):
        """Data parallel, sharded schedule: the parameter all-gathers of the last optimizer step may still be in
        flight on the collective stream - everything that reads the parameters outside run() waits for them first."""
        self._schedule.wait_all()

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        self._dp_finish()
        self._sync_buffers_from_engine()
        sd = destination if destination is not None else {}
        for name, p in self.named_parameters():
            sd[prefix + name] = p if keep_vars else p.detach()
        for b, nm in self._BUF_NAMES.items():
            if b in self._buffers:
                sd[prefix + nm] = self._buffers[b]
        return sd

    def load_state_dict(self, state_dict, strict=True, assign=False):
        own = dict(self.named_parameters())
        missing = [k for k in own if k not in state_dict]
        unexpected = []
        inv = {v: k for k, v in self._BUF_NAMES.items()}
        with torch.no_grad():
            for k, v in state_dict.items():
                if k in own:
                    own[k].copy_(v.reshape(own[k].shape))
                elif k in inv and inv[k] in self._buffers:
                    self._buffers[inv[k]].copy_(v)
                else:
                    unexpected.append(k)
        self._push_buffers_to_engine()
        self._weights_epoch += 1
        if strict and (missing or [u for u in unexpected if "_lead" not in u and "eye" not in u
                                   and "residual_offsets" not in u]):
            raise RuntimeError(f"state_dict mismatch: missing {missing}, unexpected {unexpected}")
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    # ---- device placement / engine ---------------------------------------------------------
    def _apply(self, fn, recurse=True):
        # .to(device) / .float() ...: let nn.Module move the parameter tensors (views into the
        # engine's flat buffer are copied out by this), then drop the engines; one is rebuilt
        # lazily on the next run() and the values (and the Adam moments) are copied back in.
        if self._engine is not None:
            self._refuse_while_averaged_in("model.to() / a dtype change")
            self._refuse_mid_group("model.to() / a dtype change")
            self._dp_finish()
            self._sync_buffers_from_engine()
            self._save_opt_carry()
        out = super()._apply(fn, recurse)
        self._engine = None
        self._engines = {}
        self._device = next(iter(self._parameters.values())).device
        if self._opt_carry is not None:
            self._opt_carry = self._opt_carry.to(self._device)
        self._anchor = torch.zeros((), requires_grad=True, device=self._device)
        return out

    def _refuse_while_averaged_in(self, what):
        """Inside FusedAdam.averaged_weights() the swap back is a launch on the live engine: the engine may change (another
        batch size, sample()), it may not go away."""
        if self._engine.averaged_in:
            raise L.AewError(f"{what} inside FusedAdam.averaged_weights(): leave the context first")

    def _drop_engine(self):
        if self._engine is not None:
            self._dp_finish()
            self._pull_params_to_cpu()
            self._save_opt_carry()
        self._engine = None
        self._engines = {}

    def _save_opt_carry(self):
        """The optimizer state lives in the engine's flat buffers; keep it when the engine goes away (model.to(),
        override(), a different batch size, sample()), so it survives exactly like torch.optim.Adam's per-parameter state
        does in the reference's save / restore flow (checkpoint.py:82-102)."""
        eng = self._engine
        # an engine that has neither stepped nor holds an average has nothing a carry (a restored checkpoint) lacks.
        # While the average is swapped in, `avg` holds the raw parameters and the flag travels along: that happens only
        # between two engines (another batch size inside averaged_weights()) - to() and override() are refused there
        if eng is not None and (eng.step_count > 0 or eng.avg_live or self._opt_carry is None):
            # sharded data parallel: unless the state was just gathered this rank's copy is valid for its own shards only
            # - enough to continue training on a rebuilt engine (same shard layout), not to write a checkpoint
            self._opt_carry = eng.opt_state(clone=True)._replace(complete=self._opt_complete(eng))

    def _opt_complete(self, eng) -> bool:
        return self._dp is None or self._dp.moments_complete(eng)

    def _load_opt_state(self, st: OptState):
        """FusedAdam.load_state_dict: a complete state that every rank restores - into the carry, and into the engine
        where one is live."""
        self._opt_carry = st.to(self._device)
        if self._engine is not None:
            self._engine.load_opt_state(self._opt_carry)
        if self._dp is not None:
            self._dp.moments_complete_at(st.step)

    def _opt_state(self, avg: bool = False) -> Optional[OptState]:
        """The optimizer state from the live engine (views), else from the carry, else None.  avg=False: for a reader of
        step / m / v - they stay readable while the average is swapped in (the swap does not touch them).  avg=True: for a
        reader of the average - None also where there is none, refused while it is swapped in."""
        eng = self._engine
        st = self._opt_carry if eng is None else eng.opt_state(clone=False)._replace(complete=self._opt_complete(eng))
        if st is None or (avg and st.avg is None):
            return None
        if avg and st.averaged_in:
            raise L.AewError("the averaged weights are swapped in (FusedAdam.averaged_weights()): leave the context "
                             "before reading optimizer state")
        if not st.complete:
            raise L.AewError("the optimizer state is sharded across the data-parallel ranks (each rank holds the Adam "
                             "moments and the averaged weights of its own 1/world): call dp.sync_optimizer_state(model) - "
                             "or checkpoint.save(...) - on ALL ranks before reading it on any of them (and before the "
                             "engine goes away: what the model then carries stays this rank's shards only)")
        return st

    def _pull_params_to_cpu(self):
        eng = self._engine
        self._dp_finish()
        self._sync_buffers_from_engine()
        with torch.no_grad():
            for name, pname in self._pnames:
                self._parameters[pname].data = eng.ps.view(name).detach().clone()

    def _sync_buffers_from_engine(self):
        eng = self._engine
        if eng is not None and eng.bn_type == "vqvae-ema":
            self._buffers["bn_emb"] = eng.emb.detach().clone()
            self._buffers["bn_ema_numer"] = eng.ema_numer.detach().clone()
            self._buffers["bn_ema_denom"] = eng.ema_denom.detach().clone()
            self._buffers["bn_ind_hist"] = eng.ind_hist.detach().clone()

    def _push_buffers_to_engine(self):
        eng = self._engine
        if eng is not None and eng.bn_type == "vqvae-ema":
            eng.emb.copy_(self._buffers["bn_emb"])
            eng.ema_numer.copy_(self._buffers["bn_ema_numer"])
            eng.ema_denom.copy_(self._buffers["bn_ema_denom"])
            eng.ind_hist.copy_(self._buffers["bn_ind_hist"])

    def _ensure_engine(self, B: int):
        eng = self._engine
        if eng is not None and eng.B == B:
            return eng
        if eng is not None:                                      # (before anything is changed)
            self._refuse_mid_group(f"a batch of {B} windows (the group's engine has {eng.B}; sample() uses 1)")
        if self._device.type != "cuda":
            raise L.AewError("this model executes only through the HIP library on an MI355X; "
                             "move it to a cuda device first (no CPU execution path exists)")
        L.load()
        if eng is not None:
            self._dp_finish()
            # another batch size (e.g. sample() uses B = 1 between training steps): parameters, EMA buffers and
            # optimizer state move to the other engine; engines are kept per batch size so that switching back does
            # not rebuild plans and graphs
            self._pull_params_to_cpu()
            self._save_opt_carry()
        new = self._engines.get(B)
        if new is None:
            new = TrainEngine(self.hps, B, self._device, n_win=self.window_batch_size, **self._opts)
            self._engines[B] = new
        if eng is not None and eng.eval_acc is not None:         # the evaluation record moves along (device copies)
            new.eval_plans()
            new.eval_acc.copy_(eng.eval_acc)
            new.eval_hist.copy_(eng.eval_hist)
        if eng is not None and self._eval_ev is not None and self._eval_ev._started:
            new.eval_group_reset(eng.eval_G)                     # ... and so does the grouped one (eval_win is per batch)
            for dst, src in ((new.eval_gacc, eng.eval_gacc), (new.eval_ghist, eng.eval_ghist), (new.eval_gtot, eng.eval_gtot)):
                if src is not None:
                    dst.copy_(src)
        return self._adopt_engine(new)

    def _adopt_engine(self, eng):
        """Make `eng` the live engine: the parameters become views into its flat buffer (values preserved), the buffers
        and the carried optimizer state move in."""
        with torch.no_grad():
            for name, pname in self._pnames:
                p = self._parameters[pname]
                view = eng.ps.view(name)
                view.copy_(p.data.to(self._device))
                p.data = view
                p.grad = eng.ps.view(name, grad=True)
        self._grads_cleared = True                               # gradients do not move between engines
        self._engine = eng
        self._weights_epoch += 1
        self._push_buffers_to_engine()
        if self._opt_carry is not None:                          # (none: the first engine of a model - it starts at zero)
            eng.load_opt_state(self._opt_carry)
        if self._dp is not None:
            self._dp.prepare_vae(eng)
        if eng.bn_type == "vae":
            eng.set_anneal_weight(float(self.objective.anneal_weight))
        return eng

    # ---- the hot path ----------------------------------------------------------------------
    def run(self, wav, mel, voice, jitter, eps=None):
        """(wav, mel, voice, jitter) -> (pred, target, loss)   [chassis.py:152]

        wav (B, enc_in_len) float32 holding mu-law ints; mel (B, n_mel, frames) float32;
        voice (B,) int64; jitter (B, >= embed_len) int64.  pred (B, Q, w-1) logits, target
        (B, w-1), loss scalar with a grad_fn whose backward fills every parameter's .grad."""
        B = wav.shape[0]
        eng = self._ensure_engine(B)
        self._schedule.wait_params()
        eng.set_inputs(wav, mel, voice, jitter, eps=eps)
        loss = _StepFn.apply(self._anchor, self)
        w, g = eng.n_win, eng.geom
        pred = eng.logits()[:, :w - 1, :].permute(0, 2, 1)
        target = wav[:, g.wav_out_off + 1: g.wav_out_off + w]
        self._fill_forward_metrics(eng)
        return pred, target, loss

    def evaluate(self, wav, mel, voice, jitter, eps=None, group=None):
        """The loss of a held-out batch, computed without a training step: nothing the next run() / backward() / step()
        reads is written - not the EMA statistics, the code histogram, the diagnostics behind `objective.metrics`, the
        loss word, parameters, gradients or optimizer state (TrainEngine.evaluate).  Inside
        `FusedAdam.averaged_weights()` it uses the averaged weights.  It does overwrite the activations: a pending
        `loss.backward()` of an earlier run() raises afterwards.  Every call also folds the batch into the running record
        `model.evaluation()` reads; outside such a block that record is simply never read.  No collectives, no host
        synchronisation.  Returns the 0-d device loss.  Inside `model.evaluation(by="voice")` the batch is also folded
        per window into the grouped record by its `voice` ids; inside `model.evaluation(groups=G)` by `group`, an int64
        (B,) tensor of ids in [0, G) (a window with an id outside is dropped from the grouped record and counted as
        dropped) - one more small op, still no host synchronisation."""
        ev = self._eval_ev
        grp = ev._group if ev is not None else None
        if group is not None and (grp is None or grp[0] != "group"):
            raise L.AewError("evaluate(group=...) needs an enclosing `with model.evaluation(groups=G)` block")
        if grp is not None and grp[0] == "group":
            if group is None:
                raise L.AewError("evaluate() inside model.evaluation(groups=G) needs group=ids, one id per window")
            if tuple(group.shape) != (wav.shape[0],):
                raise L.AewError(f"evaluate(): group ({wav.shape[0]},) expected (one id per window), got {tuple(group.shape)}")
        with torch.no_grad():
            eng = self._ensure_engine(wav.shape[0])
            self._dp_finish()
            eng.set_inputs(wav, mel, voice, jitter, eps=eps)
            eng.eval_grouping = grp is not None
            if grp is not None:
                if not ev._started:                                  # the block's first batch starts the grouped record
                    eng.eval_group_reset(grp[1])
                    ev._started = True
                eng.in_group.copy_(voice if grp[0] == "voice" else group)
            return eng.evaluate().clone()

    @contextlib.contextmanager
    def evaluation(self, by: Optional[str] = None, groups: Optional[int] = None):
        """`with model.evaluation() as ev:` - the record starts at zero, every model.evaluate() inside adds its batch,
        `ev.result()` returns the means (Evaluator.result).  The record follows the model when another batch size makes
        another engine the live one.

        `model.evaluation(by="voice")` also keeps the record per voice (G = hps.n_speakers groups, the ids are the
        `voice` argument of each evaluate()); `model.evaluation(groups=G)` keeps it per caller-supplied id
        (`evaluate(..., group=ids)`: gender, utterance, dataset).  Then `ev.by_group()`, `ev.information()`,
        `ev.counts()` and `ev.windows()` read it (Evaluator); `ev.result()` is what it is without grouping, bit for
        bit.  With no arguments nothing of this exists or runs."""
        if by is not None and groups is not None:
            raise L.AewError("evaluation(): give by='voice' or groups=G, not both")
        if by is not None and by != "voice":
            raise L.AewError(f"evaluation(by={by!r}): only by='voice' is known; use groups=G with evaluate(group=ids) "
                             "for any other labelling")
        if groups is not None and int(groups) < 1:
            raise L.AewError(f"evaluation(groups={groups}): at least one group")
        if self._eval_ev is not None:
            raise L.AewError("evaluation(): a grouping evaluation block is already open")
        if self._engine is not None and self._engine.eval_acc is not None:     # (else: the record is allocated as zeros)
            self._engine.eval_reset()
        if by is None and groups is None:
            yield Evaluator(self)
            return
        # (the grouped record is started by the block's first evaluate(): the engine may not exist yet)
        self._eval_ev = Evaluator(self, ("voice", int(self.hps.n_speakers)) if by is not None else ("group", int(groups)))
        try:
            yield self._eval_ev
        finally:
            self._eval_ev = None
            if self._engine is not None:
                self._engine.eval_grouping = False

    def forward(self, wav, mel, voice, jitter):
        """train(): logits (B, Q, w) for the batch (teacher-forced).  eval(): the reference's inference call
        (mfcc_inverter.py:80-85 -> WaveNet.forward_test, wavenet.py:367-531): generates `n_replicas` continuations
        of the single input window and returns (1 + n_replicas, dec_in_len) mu-law values, row 0 = the input."""
        if not self.training:
            return self.sample(wav, mel, voice, jitter)
        eng = self._ensure_engine(wav.shape[0])
        self._dp_finish()
        eng.set_inputs(wav, mel, voice, jitter)
        eng.forward(self._ema_allreduce)
        return eng.logits().permute(0, 2, 1)

    def _draw_records(self, what, draw, n):
        """The draw controls of n replicas / rows / utterances: None when there are none or all are neutral (no table is
        passed: the sampler launches what it launched before), else a list of n sampler.Draw.  `draw` None: model.draw."""
        from . import sampler as S
        if draw is None:
            draw = self.draw
        if draw is None:
            return None
        if isinstance(draw, S.Draw):
            draw = [draw] * n
        else:
            draw = list(draw)
            if len(draw) != n or not all(isinstance(d, S.Draw) for d in draw):
                raise L.AewError(f"{what}: draw must be one Draw or a sequence of {n} Draws, got {draw!r}")
        return None if all(d.is_neutral() for d in draw) else draw

    def sample(self, wav, mel, voice, jitter, n_prime: Optional[int] = None, seed: Optional[int] = None, draw=None):
        """Autoregressive generation on the persistent-kernel sampler (sampler.py).  The first n_prime positions of
        the decoder window are fed from `wav` (default: receptive field + 1, like the reference, which starts
        drawing at base_global_rf, wavenet.py:423-431); the rest are drawn.  One input window (B = 1); replicas are
        parallel streams (wavenet.py:378-381).  draw: the draw controls (sampler.Draw: temperature, top-k, nucleus,
        greedy) of every replica, or a sequence with one per replica; default model.draw; None or neutral: the plain
        draw, bit for bit."""
        if wav.shape[0] != 1:
            raise L.AewError("sampling takes one window; replicas come from set_n_replicas()")
        R = max(1, int(self.n_replicas))
        recs = self._draw_records("sample()", draw, R)
        self._dp_finish()
        with torch.no_grad():
            eng = self._ensure_engine(1)
            eng.set_inputs(wav, mel, voice, jitter)
            cond, bias = eng.conditioning()
            smp = self._engine_sampler(eng)
            g = eng.geom
            T, rf = g.dec_in_len, smp.g.rf()
            n16 = (R + 15) // 16 * 16
            given = wav[:, g.trim_dec_in[0]:g.trim_dec_in[0] + T].to(torch.int32)
            forced = given.expand(n16, -1).clone()
            forced[:, min(T, rf + 1 if n_prime is None else max(1, n_prime)):] = -1
            if seed is None:
                seed, self.sample_seed = self.sample_seed, self.sample_seed + 1
            out, _ = smp.generate(cond.expand(n16, -1, -1).contiguous(), bias.expand(n16, -1, -1).contiguous(),
                                  forced.contiguous(), seed=seed,
                                  draw=None if recs is None else recs + [recs[0]] * (n16 - R))
            return torch.cat([given, out[:R]], 0).float()

    def _engine_sampler(self, eng):
        """The cached sampler over the live engine's decoder.  It keeps its own packed copy of the weights: re-packed
        whenever they may have changed.  FusedAdam updates parameters by raw pointer (no tensor _version bump), hence
        the explicit counters."""
        from . import sampler as S
        stamp = (eng.serial, eng.ps.params._version, eng.weights_version, self._weights_epoch)
        if self._sampler is None or self._sampler[0] != stamp:
            self._sampler = (stamp, S.from_engine(eng))
        return self._sampler[1]

    # ---- the codes between encoder and decoder as an interface ------------------------------------------------------
    def _need_codes(self, what: str):
        if self.bn_type not in ("vqvae", "vqvae-ema"):
            raise L.AewError(f"{what} needs a model with discrete codes (bn_type vqvae or vqvae-ema); the bottleneck of "
                             f"this model is '{self.bn_type}'")

    def encode(self, mel, return_dist: bool = False):
        """mel (B, n_mel, frames) -> codes int64 (B, embed_len), a fresh tensor: the index of the nearest codebook entry
        per encoder frame (the training forward's encoder, bottleneck linear and nearest-code search; no EMA statistics,
        no histogram, no loss word is written).  return_dist=True: (codes, dist) with the (B, embed_len) distances to the
        chosen entries.  Inside `FusedAdam.averaged_weights()` it uses the averaged weights.  It overwrites the encoder
        activations: a pending `loss.backward()` of an earlier run() raises afterwards.  No host synchronisation."""
        self._need_codes("encode()")
        B = mel.shape[0]
        with torch.no_grad():
            eng = self._ensure_engine(B)
            self._dp_finish()
            eng.in_mel.copy_(mel)                                    # (the only input the plan reads)
            ind, dist = eng.encode_codes()
            codes = ind.view(B, self.embed_len).clone()
            return (codes, dist.view(B, self.embed_len).clone()) if return_dist else codes

    # ---- whole utterances: codes for any length and for a corpus ----------------------------------------------------
    def _ragged_mels(self, what, mels):
        """A list of (n_mel, F_u) device tensors -> (flat, frames, bases): the ragged fp32 buffer of the arrays one behind
        the other, the frame count of each and the element offset it starts at."""
        mels = list(mels)
        n_mel = self._opts["n_mel"] or 3 * self.hps.n_mfcc
        for m in mels:
            if m.dim() != 2 or m.shape[0] != n_mel or m.device.type != "cuda":
                raise L.AewError(f"{what}: ({n_mel}, frames) device tensors expected, got {tuple(m.shape)} on '{m.device}'")
        frames = [int(m.shape[1]) for m in mels]
        bases = [0] + np.cumsum([n_mel * F for F in frames[:-1]], dtype=np.int64).tolist() if frames else []
        flat = torch.cat([m.to(torch.float32).reshape(-1) for m in mels]) if sum(frames) else \
            torch.empty(0, dtype=torch.float32, device=self._device)
        return flat, frames, bases

    def _ragged_engine(self, what, U, voice, batch):
        """The batch and voice checks of a call over U whole utterances -> (B, voice as an int64 tensor or None, the engine
        of B rows)."""
        if batch is not None and int(batch) < 1:
            raise L.AewError(f"{what}: batch must be at least 1, got {batch}")
        B = int(batch) if batch is not None else (self._engine.B if self._engine is not None else int(self.hps.n_batch))
        if voice is not None:
            voice = torch.as_tensor(voice, dtype=torch.int64)
            if tuple(voice.shape) != (U,):
                raise L.AewError(f"{what}: voice ({U},) expected (one per utterance), got {tuple(voice.shape)}")
        with torch.no_grad():
            eng = self._ensure_engine(B)
            self._dp_finish()
        return B, voice, eng

    def _corpus_chunks(self, corpus, max_frames_per_chunk):
        """The utterances of a `corpus.DeviceCorpus` in chunks of at most max_frames_per_chunk mel frames (one utterance at
        least) -> (the resident sound as a 1-D tensor of samples, [[indices into corpus.samples of one chunk]])."""
        if corpus.snd is None:
            corpus._need_device()
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[corpus.snd_bytes]
        snd = corpus.snd[:corpus.n_snd * corpus.snd_bytes].view(dt)
        mf = self._utterance_mfcc()
        chunks, cur, held = [], [], 0
        for i, sam in enumerate(corpus.samples):
            F = max(0, mf.n_frames(int(sam[2]) - int(sam[1])))
            if cur and held + F > int(max_frames_per_chunk):
                chunks.append(cur)
                cur, held = [], 0
            cur.append(i)
            held += F
        if cur:
            chunks.append(cur)
        return snd, chunks

    def _cat(self, tensors, dtype):
        return torch.cat(tensors) if tensors else torch.empty(0, dtype=dtype, device=self._device)

    def _corpus_codes(self, corpus, parts, return_dist):
        """The `codes.UtteranceCodes` of the chunks `parts`, one behind the other, with the corpus's voices and names."""
        from . import codes as CD
        offsets = [0]
        for p in parts:
            at = offsets[-1]
            offsets += [at + o for o in p._off[1:]]
        sams = corpus.samples
        voice = torch.tensor([int(s[0]) for s in sams], dtype=torch.int64)
        names = [str(s[3]) for s in sams] if all(len(s) > 3 for s in sams) else None
        return CD.UtteranceCodes(self._cat([p.codes for p in parts], torch.int64), torch.tensor(offsets, dtype=torch.int64),
                                 dist=self._cat([p.dist for p in parts], torch.float32) if return_dist else None,
                                 voice=voice, names=names)

    def _encode_ragged(self, what, flat, frames, bases, voice, batch, return_dist, names):
        """flat: the ragged fp32 buffer of the utterances' (n_mel, frames[u]) arrays at the element offsets `bases`."""
        from . import codes as CD
        B, voice, eng = self._ragged_engine(what, len(frames), voice, batch)
        with torch.no_grad():
            E, s, rf, _ = G.utterance_geometry(eng.geom)
            plan = CD.tile_plan(frames, E, s, rf, B)
            codes = torch.empty(plan.n_codes, dtype=torch.int64, device=eng.device)
            dist = torch.empty(plan.n_codes, dtype=torch.float32, device=eng.device) if return_dist else None
            eng.encode_tiles(flat, plan.table(bases), codes, dist)
        return CD.UtteranceCodes(codes, torch.from_numpy(plan.offsets), dist=dist, voice=voice, names=names)

    def encode_utterances(self, mels, voice=None, batch=None, return_dist: bool = False, names=None):
        """mels: a list of (n_mel, F_u) device tensors of ANY frame counts -> `codes.UtteranceCodes`: the codes of each
        whole utterance, flat (int64 `codes`, `offsets` of size U + 1; `dist` with return_dist=True; `voice` / `names`
        carried along).  An utterance of F frames has 0 codes below the encoder's receptive field rf, else
        (F - rf) // s + 1 (geometry.utterance_geometry).  The encoder is a chain of valid convolutions, so the utterance
        is cut into overlapping windows of the engine's fixed geometry at hop s * embed_len, zero-padded behind its last
        frame, and only codes whose receptive field lies inside real frames are kept: frame for frame the bits one run
        over the whole utterance gives.  The windows of all utterances are packed into batches of `batch` rows (default:
        the live engine's B); the last batch is padded with idle rows.  The work list is `codes.tile_plan` of the frame
        counts - the device is never asked for a size.  Otherwise the rules of encode(): VQ bottlenecks only; no
        codebook, EMA statistic, histogram, loss or metric word is written; inside `FusedAdam.averaged_weights()` the
        averaged weights are used; a pending `loss.backward()` raises afterwards; no host synchronisation and no
        collective (under data parallel each rank encodes what it is given)."""
        self._need_codes("encode_utterances()")
        flat, frames, bases = self._ragged_mels("encode_utterances()", mels)
        return self._encode_ragged("encode_utterances()", flat, frames, bases, voice, batch, return_dist, names)

    def _utterance_mfcc(self):
        from .mfcc import DeviceMfcc
        h = self.hps
        if self._utt_mfcc is None or self._utt_mfcc.dev != self._device:
            self._utt_mfcc = DeviceMfcc(self._device, h.sample_rate, h.mfcc_win_sz, h.mfcc_hop_sz, h.n_mels, h.n_mfcc)
        if self._utt_mfcc.n_out != (self._opts["n_mel"] or 3 * h.n_mfcc):
            raise L.AewError(f"encode_wavs(): the MFCC front-end yields {self._utt_mfcc.n_out} channels, the encoder takes "
                             f"{self._opts['n_mel']}")
        return self._utt_mfcc

    def encode_wavs(self, wavs, voice=None, batch=None, return_dist: bool = False, names=None):
        """wavs: a list of 1-D device tensors of mu-law values, whole utterances of any lengths -> `codes.UtteranceCodes`.
        The MFCC of each WHOLE utterance is computed on the device (one AEW_OP_MFCC record per utterance,
        DeviceMfcc.ragged: the dB floor and the delta edges are the utterance's, the reference's definition when its
        loader hands over entire files) straight into the ragged buffer encode_utterances() tiles."""
        self._need_codes("encode_wavs()")
        if self._device.type != "cuda":
            raise L.AewError("encode_wavs() runs on an MI355X only; move the model to a cuda device first")
        flat, frames, bases = self._utterance_mfcc().ragged(wavs)
        return self._encode_ragged("encode_wavs()", flat, frames, bases, voice, batch, return_dist, names)

    def encode_corpus(self, corpus, batch=None, max_frames_per_chunk: int = 1 << 16, return_dist: bool = False):
        """Tokenise a `corpus.DeviceCorpus`: every utterance of `corpus.samples`, in that order, straight from the
        resident sound bytes, as encode_wavs() does -> `codes.UtteranceCodes` with `voice` = the samples' voice_index and
        `names` = their file_path (where the records carry one).  The utterances are taken in chunks of at most
        max_frames_per_chunk mel frames (one utterance at least), which bounds the memory held besides the result;
        every utterance is encoded on its own, so the chunking does not change a bit."""
        self._need_codes("encode_corpus()")
        snd, chunks = self._corpus_chunks(corpus, max_frames_per_chunk)
        sams = corpus.samples
        parts = [self.encode_wavs([snd[int(sams[i][1]):int(sams[i][2])] for i in ch], batch=batch, return_dist=return_dist)
                 for ch in chunks]
        return self._corpus_codes(corpus, parts, return_dist)

    # ---- whole utterances: the code sequence chosen jointly ---------------------------------------------------------
    def _segment_ragged(self, what, flat, frames, bases, penalty, voice, batch, return_dist, names, return_info):
        from . import codes as CD
        lam = CD._penalties(penalty, len(frames), what)                      # (refused before anything runs)
        B, voice, eng = self._ragged_engine(what, len(frames), voice, batch)
        with torch.no_grad():
            if eng.bn.K > L.SEG_MAX_K:
                raise L.AewError(f"{what}: a codebook of at most {L.SEG_MAX_K} entries expected, this one has {eng.bn.K}")
            E, s, rf, _ = G.utterance_geometry(eng.geom)
            plan = CD.tile_plan(frames, E, s, rf, B)
            codes, dist, info = eng.segment_tiles(flat, plan.table(bases), plan.offsets, lam, return_dist)
        uc = CD.UtteranceCodes(codes, torch.from_numpy(plan.offsets), dist=dist, voice=voice, names=names)
        return (uc, info) if return_info else uc

    def segment_utterances(self, mels, penalty, voice=None, batch=None, return_dist: bool = False, names=None,
                           return_info: bool = False):
        """encode_utterances() with the code sequence of each utterance chosen JOINTLY: the labelling that minimises
        sum over frames of the distance to the chosen entry + penalty * (number of code changes), a Viterbi pass over the
        codebook on the device (AEW_OP_CODE_SEGMENT; include/aewavenet.h states the rule bit for bit).  penalty: one float
        or one per utterance, >= 0; 0 gives encode_utterances()'s codes and distances bit for bit, inf one code per
        utterance, in between it trades bitrate against distortion.  The distance is the bottleneck's own (scaled_l2 for
        vqvae-ema, sq_l2 for vqvae) to the live codebook, which may hold at most 4096 entries.  -> `codes.UtteranceCodes`
        (`dist` with return_dist=True: the distance of every frame to ITS chosen entry), so units(), save(),
        decode_utterances(), score_utterances(codes=...), align.edit_distance() and voice_information() take it as it is;
        return_info=True: (UtteranceCodes, `codes.Segmentation`) with the cost, the segment count and the penalty of every
        utterance and the count of utterances whose cost is not finite, on the device.  Besides the result the call holds
        the encoder outputs of all utterances and a workspace of n_codes * K * 4 bytes of local costs (segment_corpus()
        bounds it).  Otherwise the rules of encode_utterances(): VQ bottlenecks only; no codebook, EMA statistic,
        histogram, loss or metric word is written; inside `FusedAdam.averaged_weights()` the averaged weights are used; no
        host synchronisation."""
        self._need_codes("segment_utterances()")
        flat, frames, bases = self._ragged_mels("segment_utterances()", mels)
        return self._segment_ragged("segment_utterances()", flat, frames, bases, penalty, voice, batch, return_dist, names,
                                    return_info)

    def segment_wavs(self, wavs, penalty, voice=None, batch=None, return_dist: bool = False, names=None,
                     return_info: bool = False):
        """segment_utterances() from the waveforms: the whole-utterance MFCC of encode_wavs(), then the joint choice."""
        self._need_codes("segment_wavs()")
        if self._device.type != "cuda":
            raise L.AewError("segment_wavs() runs on an MI355X only; move the model to a cuda device first")
        flat, frames, bases = self._utterance_mfcc().ragged(wavs)
        return self._segment_ragged("segment_wavs()", flat, frames, bases, penalty, voice, batch, return_dist, names, return_info)

    def segment_corpus(self, corpus, penalty, batch=None, max_frames_per_chunk: int = 1 << 15, return_dist: bool = False,
                       return_info: bool = False):
        """Segment a `corpus.DeviceCorpus` as encode_corpus() tokenises it: every utterance of `corpus.samples`, in that
        order, in chunks of at most max_frames_per_chunk mel frames (one utterance at least).  penalty: one float or one
        per utterance.  The utterances are independent, so the chunking does not change a bit; it bounds what a chunk
        holds besides the result - above all the local costs, codes_in_chunk * K * 4 bytes (at most
        max_frames_per_chunk * K * 4: 512 MiB at the default and K = 4096)."""
        from . import codes as CD
        self._need_codes("segment_corpus()")
        snd, chunks = self._corpus_chunks(corpus, max_frames_per_chunk)
        sams = corpus.samples
        lam = CD._penalties(penalty, len(sams), "segment_corpus()")
        parts = [self.segment_wavs([snd[int(sams[i][1]):int(sams[i][2])] for i in ch], lam[ch], batch=batch,
                                   return_dist=return_dist, return_info=True) for ch in chunks]
        uc = self._corpus_codes(corpus, [p for p, _ in parts], return_dist)
        if not return_info:
            return uc
        n_bad = torch.stack([i.n_bad for _, i in parts]).sum(0) if parts else torch.zeros(1, dtype=torch.int32, device=self._device)
        info = CD.Segmentation(self._cat([i.cost for _, i in parts], torch.float32), self._cat([i.n_segments for _, i in parts], torch.int32),
                               self._cat([i.penalty for _, i in parts], torch.float32), n_bad.to(torch.int32))
        return uc, info

    def zero_amplitude_code(self) -> int:
        """The mu-law value a sample of amplitude 0 encodes to (codes.mu_encode with this model's n_quant)."""
        from . import codes as CD
        return int(CD.mu_encode(torch.zeros(1), self.n_quant)[0])

    def decode(self, codes, voice, prime=None, n_prime: Optional[int] = None, seed: Optional[int] = None, jitter=None,
               draw=None):
        """codes (B, embed_len) int64, voice (B,) -> (B, dec_in_len) float32 mu-law values: the decoder conditioned on the
        GIVEN codes in the given voices, one sampler stream per row (padded to a multiple of 16 streams by repeating row
        0; the pad streams are dropped).  The first n_prime positions (default: receptive field + 1, as in sample())
        are forced to prime[:, :n_prime] - mu-law values (B, >= n_prime) - or, without `prime`, to the value silence
        encodes to (zero_amplitude_code()); the rest are drawn.  jitter (B, >= embed_len): the conditioning gather's
        index, default the identity (no jitter at inference).  seed as in sample().  draw: one sampler.Draw for every
        row or a sequence with one per row (pad streams take row 0's), default model.draw.  A code outside [0, K) raises
        AewError with the count before the sampler starts (the lookup never follows it)."""
        self._need_codes("decode()")
        E = self.embed_len
        if codes.dim() != 2 or codes.shape[1] != E or codes.dtype != torch.int64:
            raise L.AewError(f"decode(): codes (B, {E}) int64 expected, got {tuple(codes.shape)} {codes.dtype}")
        B = codes.shape[0]
        if tuple(voice.shape) != (B,):
            raise L.AewError(f"decode(): voice ({B},) expected (one per row of codes), got {tuple(voice.shape)}")
        if jitter is not None and (jitter.dim() != 2 or jitter.shape[0] != B or jitter.shape[1] < E):
            raise L.AewError(f"decode(): jitter ({B}, >= {E}) expected, got {tuple(jitter.shape)}")
        recs = self._draw_records("decode()", draw, B)
        with torch.no_grad():
            eng = self._ensure_engine(B)
            self._dp_finish()
            dev = eng.device
            eng.in_voice.copy_(voice)
            eng.in_jitter.copy_(torch.arange(E, device=dev).expand(B, -1) if jitter is None else jitter[:, :E])
            cond, bias = eng.codes_to_conditioning(codes.to(dev))
            bad = int(eng.codes_bad[0].item()) & 0xFFFFFFFF          # (generation synchronises anyway)
            if bad:
                raise L.AewError(f"decode(): {bad} of the {B * E} codes lie outside the codebook [0, {eng.K}); nothing was "
                                 "generated")
            smp = self._engine_sampler(eng)
            T, rf = eng.geom.dec_in_len, smp.g.rf()
            n_forced = min(T, rf + 1 if n_prime is None else max(1, n_prime))
            n16 = (B + 15) // 16 * 16
            forced = torch.full((n16, T), -1, dtype=torch.int32, device=dev)
            if prime is None:
                forced[:, :n_forced] = self.zero_amplitude_code()
            else:
                if prime.dim() != 2 or prime.shape[0] != B or prime.shape[1] < n_forced:
                    raise L.AewError(f"decode(): prime ({B}, >= {n_forced}) expected, got {tuple(prime.shape)}")
                forced[:B, :n_forced] = prime[:, :n_forced].to(device=dev, dtype=torch.int32)
                forced[B:] = forced[0]
            rows = torch.arange(n16, device=dev)
            rows[B:] = 0                                             # pad streams repeat row 0
            if seed is None:
                seed, self.sample_seed = self.sample_seed, self.sample_seed + 1
            out, _ = smp.generate(cond[rows].contiguous(), bias[rows].contiguous(), forced, seed=seed,
                                  draw=None if recs is None else recs + [recs[0]] * (n16 - B))
            return out[:B].float()

    def convert(self, wav, mel, voice_to, n_prime: Optional[int] = None, seed: Optional[int] = None, jitter=None,
                draw=None):
        """Voice conversion: decode(encode(mel), voice_to, prime=<the decoder window of wav>).  wav (B, enc_in_len), mel
        (B, n_mel, frames), voice_to (B,) - or (V,) with B = 1: that one window is decoded in V voices at once, as V
        streams.  Returns (B or V, dec_in_len) float32 mu-law values whose first n_prime columns are the window's.  draw as
        in decode(): one Draw, or one per output row (per voice with one window)."""
        self._need_codes("convert()")
        B, T, o = wav.shape[0], self.dec_in_len, int(self.trim_dec_in[0])
        V = voice_to.shape[0] if voice_to.dim() == 1 else -1
        if V != B and not (B == 1 and V >= 1):
            raise L.AewError(f"convert(): voice_to ({B},) expected, or (V,) with one window; got {tuple(voice_to.shape)} "
                             f"for {B} windows")
        codes = self.encode(mel)
        given = wav[:, o:o + T]
        if V != B:
            codes, given = codes.expand(V, -1).contiguous(), given.expand(V, -1)
        return self.decode(codes, voice_to, prime=given, n_prime=n_prime, seed=seed, jitter=jitter, draw=draw)

    # ---- whole utterances, the decoder's side: conditioning of any length from codes, generation, conversion ----------
    def _utterance_rows(self, what, codes, voice):
        """(rows: list of 1-D int64 device tensors, voices: list of ints) from an UtteranceCodes or a list of tensors."""
        from . import codes as CD
        if isinstance(codes, CD.UtteranceCodes):
            rows = [codes.row(u) for u in range(len(codes))]
            if voice is None:
                voice = codes.voice
        else:
            rows = list(codes)
        U = len(rows)
        for r in rows:
            if not torch.is_tensor(r) or r.dim() != 1 or r.dtype != torch.int64:
                raise L.AewError(f"{what}: an UtteranceCodes or a list of 1-D int64 tensors expected")
        if voice is None:
            raise L.AewError(f"{what}: voice ({U},) expected (the codes carry none)")
        voice = torch.as_tensor(voice, dtype=torch.int64).cpu().reshape(-1)
        if voice.numel() != U:
            raise L.AewError(f"{what}: voice ({U},) expected (one per utterance), got {tuple(voice.shape)}")
        voices = voice.tolist()
        nv = int(self.hps.n_speakers)
        if any(v < 0 or v >= nv for v in voices):
            raise L.AewError(f"{what}: voices must lie in [0, {nv}), got {voices}")
        return rows, voices

    def _utterance_engine(self, what, batch):
        from . import codes as CD
        self._need_codes(what)
        if self._opts.get("take_compat"):
            raise L.AewError(f"{what}: this model was built with take_compat=True, whose conditioning gather is not the "
                             "identity the tiling of whole utterances rests on")
        if batch is not None and int(batch) < 1:
            raise L.AewError(f"{what}: batch must be at least 1, got {batch}")
        if self._device.type != "cuda":
            raise L.AewError(f"{what} runs on an MI355X only; move the model to a cuda device first")
        cg = G.conditioning_geometry(self.geom)                      # (raises where the window cannot tile)
        B = int(batch) if batch is not None else (self._engine.B if self._engine is not None else int(self.hps.n_batch))
        eng = self._ensure_engine(B)
        self._dp_finish()
        return eng, cg

    def _check_codes(self, what, rows, K):
        """Raises for a code outside [0, K) anywhere in `rows` - before anything is generated (one read of the device)."""
        flat = [r for r in rows if r.numel()]
        if flat:
            flat = torch.cat([r.to(self._device) for r in flat])
            bad = int(((flat < 0) | (flat >= K)).sum())
            if bad:
                raise L.AewError(f"{what}: {bad} of the {flat.numel()} codes lie outside the codebook [0, {K}); nothing was "
                                 "generated")

    def _conditioning_of(self, eng, cg, rows, voices, n_streams):
        """cond (n_streams, T_max, Cp) bf16 / bias (n_streams, NL, 2 * Dp) fp32 / lengths for the utterances `rows`, stream
        u = utterance u; the streams behind them stay zero."""
        from . import codes as CD
        plan = CD.cond_tile_plan([r.numel() for r in rows], cg.E, cg.S, cg.T, cg.trim0, eng.B, cg.L)
        d, dev = eng.dec, eng.device
        cond = torch.zeros(n_streams, plan.pitch, d.Cp, dtype=torch.bfloat16, device=dev)
        bias = torch.zeros(n_streams, d.NL, 2 * d.Dp, dtype=torch.float32, device=dev)
        bases = np.concatenate([[0], np.cumsum(plan.n_codes)])[:-1]
        if plan.n_rows:
            flat = torch.cat([r.to(dev) for r in rows])
            eng.conditioning_tiles(flat, plan.table(bases, voices), cond, bias)
        return cond, bias, plan.lengths

    def utterance_conditioning(self, codes, voice=None, batch=None):
        """The decoder's conditioning of WHOLE utterances from their codes: `codes` a `codes.UtteranceCodes` (its `voice`
        is the default) or a list of 1-D int64 tensors of any lengths, `voice` (U,) -> (cond bf16 (U16, T_max, Cp), bias
        fp32 (U16, NL, 2 * Dp), lengths int64 (U,) on the host): stream u holds the L(N_u) = lengths[u] conditioning rows
        of utterance u - 320 N - 2172 at the reference strides, 0 below 7 codes - and zeros behind them; U16 is U rounded
        up to a multiple of 16 (the sampler's stream count), T_max the longest length.  The conditioning chain (codebook
        row, identity gather, LC conv, transposed-conv upsamplers) is shift-invariant and valid, so each utterance is cut
        into overlapping windows of the engine's fixed geometry (geometry.conditioning_geometry; work list:
        codes.cond_tile_plan), run through the unchanged conditioning plan `batch` windows at a time, and the rows each
        window owns are stitched: row for row the bits a run over the whole code sequence gives.  Row q of stream u
        belongs to sample o + q of the utterance's waveform, o = conditioning_geometry(...).o.  The result takes
        U16 * T_max * Cp * 2 bytes.  The rules of decode() hold; a code outside [0, K) raises AewError."""
        what = "utterance_conditioning()"
        eng, cg = self._utterance_engine(what, batch)
        rows, voices = self._utterance_rows(what, codes, voice)
        with torch.no_grad():
            self._check_codes(what, rows, eng.K)
            cond, bias, lengths = self._conditioning_of(eng, cg, rows, voices, max(16, -(-len(rows) // 16) * 16))
        return cond, bias, torch.from_numpy(lengths.copy())

    def decode_utterances(self, codes, voice=None, prime=None, n_prime: Optional[int] = None, seed: Optional[int] = None,
                          batch=None, draw=None):
        """Generate whole utterances from their codes: `codes` / `voice` / `batch` as in utterance_conditioning() -> a
        list of U float32 tensors of mu-law values, the u-th of L(N_u) samples (empty where L(N_u) = 0: under 7 codes at
        the reference strides; such an utterance takes no stream).  Element q is sample o + q of the waveform the codes
        were encoded from.  `prime`: a list of per-utterance mu-law tensors aligned to conditioning position 0 (that is
        wav[o:]); the first n_prime positions (default: receptive field + 1, as in decode(); clipped to L_u) are forced to
        it - without `prime`, to zero_amplitude_code() - and the rest are drawn.

        Streams.  codes.stream_groups(lengths, seed) states, as a pure function, what runs where: the utterances with
        L > 0 are ordered longest first (stable: equal lengths keep their input order), group g takes the 16 from
        position 16 g on, utterance k of a group is stream slot k of ONE Sampler.generate call with seed `seed + g` over
        T_max = the group's longest length.  Shorter streams are padded with zero conditioning and their tails dropped;
        slots a group leaves empty repeat its first utterance and are dropped.  Results come back in input order, and two
        calls with the same seed agree bit for bit.  seed=None takes sample_seed and advances it by the group count.

        draw: one sampler.Draw for every utterance, or a sequence with one per utterance (default model.draw).  A record
        follows its utterance into the stream slot stream_groups assigns; an empty slot takes the record of the
        utterance it repeats.  Groups, seeds and order do not depend on it, and neutral records change no bit.

        Memory: the conditioning of one group is 16 * T_max * Cp * 2 bytes - about 0.65 GB for ten-second utterances
        (160 000 samples) at Cp = 128.

        The rules of decode() hold: VQ bottlenecks only; a code outside [0, K) raises AewError with nothing generated; no
        codebook, EMA statistic, histogram, loss or metric word is written; inside `FusedAdam.averaged_weights()` the
        averaged weights are used; a pending `loss.backward()` raises afterwards; no collective under data parallel.  A
        model built with take_compat=True is refused."""
        from . import codes as CD
        what = "decode_utterances()"
        eng, cg = self._utterance_engine(what, batch)
        rows, voices = self._utterance_rows(what, codes, voice)
        U = len(rows)
        if prime is not None and len(prime) != U:
            raise L.AewError(f"{what}: prime must hold one tensor per utterance ({U}), got {len(prime)}")
        recs = self._draw_records(what, draw, U)
        lengths = [cg.L(r.numel()) for r in rows]
        with torch.no_grad():
            dev = eng.device
            self._check_codes(what, rows, eng.K)
            smp = self._engine_sampler(eng)
            rf = smp.g.rf()
            n_forced = [min(n, rf + 1 if n_prime is None else max(1, int(n_prime))) for n in lengths]
            for u in range(U) if prime is not None else ():
                if lengths[u] and (prime[u].dim() != 1 or prime[u].numel() < n_forced[u]):
                    raise L.AewError(f"{what}: prime[{u}] must be 1-D with at least {n_forced[u]} values, got "
                                     f"{tuple(prime[u].shape)}")
            if seed is None:
                seed = self.sample_seed
                self.sample_seed += len(CD.stream_groups(lengths, 0))
            out = [torch.empty(0, dtype=torch.float32, device=dev) for _ in range(U)]
            zero = self.zero_amplitude_code()
            for g_seed, members in CD.stream_groups(lengths, seed):
                n = len(members)
                cond, bias, got = self._conditioning_of(eng, cg, [rows[u] for u in members], [voices[u] for u in members], 16)
                assert got.tolist() == [lengths[u] for u in members]
                bad = int(eng.codes_bad[0].item()) & 0xFFFFFFFF          # (generation synchronises anyway)
                if bad:
                    raise L.AewError(f"{what}: codes outside the codebook [0, {eng.K}) were met ({bad} counted over the "
                                     "overlapping windows)")
                T_max = cond.shape[1]
                forced = torch.full((16, T_max), -1, dtype=torch.int32, device=dev)
                for k, u in enumerate(members):
                    if prime is None:
                        forced[k, :n_forced[u]] = zero
                    else:
                        forced[k, :n_forced[u]] = prime[u][:n_forced[u]].to(device=dev, dtype=torch.int32)
                if n < 16:                                               # empty slots repeat the group's first utterance
                    cond[n:], bias[n:], forced[n:] = cond[0], bias[0], forced[0]
                slot_recs = None if recs is None else [recs[u] for u in members] + [recs[members[0]]] * (16 - n)
                wav, _ = smp.generate(cond, bias, forced, seed=g_seed, draw=slot_recs)
                for k, u in enumerate(members):
                    out[u] = wav[k, :lengths[u]].float()
            return out

    def convert_utterances(self, wavs, voice_to, n_prime: Optional[int] = None, seed: Optional[int] = None, batch=None,
                           draw=None):
        """Voice conversion of whole utterances: decode_utterances(encode_wavs(wavs), voice_to, prime=[w[o:] for w in
        wavs]) with o = geometry.conditioning_geometry(model.geom).o (2235 at the reference geometry, whatever
        n_win_batch).  wavs: a list of 1-D device tensors of mu-law values; voice_to: one voice per utterance - or, with
        ONE utterance, (V,): that utterance is decoded in V voices at once, as V streams.  Returns a list of float32
        tensors; element q of an output is aligned to sample o + q of its input, and its first n_prime values are the
        input's.  draw as in decode_utterances(): one Draw, or one per output (per voice with one utterance)."""
        what = "convert_utterances()"
        self._need_codes(what)
        wavs = list(wavs)
        voice_to = torch.as_tensor(voice_to, dtype=torch.int64).cpu().reshape(-1)
        U, V = len(wavs), voice_to.numel()
        if V != U and not (U == 1 and V >= 1):
            raise L.AewError(f"{what}: voice_to ({U},) expected, or (V,) with one utterance; got {tuple(voice_to.shape)} for "
                             f"{U} utterances")
        o = G.conditioning_geometry(self.geom).o
        uc = self.encode_wavs(wavs, batch=batch)
        rows = [uc.row(u) for u in range(U)]
        prime = [w[o:] for w in wavs]
        if V != U:
            rows, prime = rows * V, prime * V
        return self.decode_utterances(rows, voice_to, prime=prime, n_prime=n_prime, seed=seed, batch=batch, draw=draw)

    # ---- whole utterances through the teacher-forced decoder: how well the decoder explains a waveform ------------------
    def score_utterances(self, wavs, voice=None, codes=None, batch=None, return_prob: bool = False, return_hit: bool = False):
        """The teacher-forced likelihood of WHOLE utterances: `wavs` a list of 1-D device tensors of mu-law values, `codes`
        a `codes.UtteranceCodes` or a list of 1-D int64 tensors (default: self.encode_wavs(wavs, batch=batch), the
        utterances' own codes), `voice` one per utterance (default: the UtteranceCodes' own) -> `codes.UtteranceScores`.
        With ONE utterance and `voice` of shape (V,), that utterance is scored under V voices at once, as V rows - speaker
        attribution in one call (the rule of convert_utterances).

        Conditioning position q of an utterance of N codes belongs to waveform sample o + q (geometry.scoring_geometry);
        the scored samples are the positions [rf + 1, n_u), n_u = min(L(N), len(wav) - o): the first rf + 1 positions are
        context only, as they are primed in decode_utterances().  `row(u)[i]` of the result is the NLL in nats of waveform
        sample `start + i`, start = o + rf + 1; `summary` holds (nll per sample, bits per sample, top-1, mean target
        probability) per utterance, `sums` the float64 record they are quotients of.  return_prob / return_hit add the
        per-sample probability of the sample that came / whether it was the arg-max class.  The utterance is cut into
        overlapping windows of the engine's geometry (work list: codes.score_tile_plan), `batch` windows at a time run
        through the unchanged conditioning and decoder plans, and the outputs each window owns are stitched: sample for
        sample the bits of any other packing of the windows into batches - and of any other batch size for which the GEMM
        launcher picks the same kernels (keep `batch` fixed where results are compared bit for bit).

        Refused with AewError before anything runs on the device: a model without discrete codes or built with
        take_compat=True, a window that holds no hop, a code outside [0, K), a waveform value outside [0, n_quant), a
        voice outside [0, n_speakers).  The rules of decode() hold: no codebook, EMA statistic, histogram, loss, metric
        or evaluation word is written; inside `FusedAdam.averaged_weights()` the averaged weights are used; a pending
        `loss.backward()` raises afterwards; no collective under data parallel."""
        from . import codes as CD
        what = "score_utterances()"
        eng, _ = self._utterance_engine(what, batch)
        sg = G.scoring_geometry(self.geom)                                 # (raises where the window cannot tile)
        wavs = list(wavs)
        for w in wavs:
            if not torch.is_tensor(w) or w.dim() != 1:
                raise L.AewError(f"{what}: wavs must be a list of 1-D tensors of mu-law values")
        nq, dev = int(self.n_quant), eng.device
        uniq, wav_bases, at = {}, [], 0                                     # (one utterance under V voices is stored once)
        for w in wavs:
            if id(w) not in uniq:
                uniq[id(w)] = (at, w)
                at += w.numel()
            wav_bases.append(uniq[id(w)][0])
        wav_flat = torch.cat([w.to(device=dev, dtype=torch.float32) for _, w in uniq.values()]) if at else \
            torch.empty(0, dtype=torch.float32, device=dev)
        if at:
            bad = int((~((wav_flat >= 0) & (wav_flat < nq))).sum())
            if bad:
                raise L.AewError(f"{what}: {bad} of the {at} waveform values lie outside [0, {nq}); nothing was scored")
        if codes is None:
            nv = int(self.hps.n_speakers)                                   # (the voices once here: the encoder runs next)
            given = [] if voice is None else torch.as_tensor(voice, dtype=torch.int64).reshape(-1).tolist()
            if not given or any(v < 0 or v >= nv for v in given):
                raise L.AewError(f"{what}: voices in [0, {nv}) expected (codes encoded here carry none), got {given}")
            if len(given) != len(wavs) and len(wavs) != 1:
                raise L.AewError(f"{what}: voice ({len(wavs)},) expected (one per utterance), or (V,) with one utterance; "
                                 f"got {len(given)} voices for {len(wavs)} utterances")
            codes = self.encode_wavs(wavs, batch=batch)
        U = len(wavs)
        n_given = len(codes)
        if n_given != U:
            raise L.AewError(f"{what}: {U} waveforms but the codes of {n_given} utterances")
        if U == 1 and voice is not None and torch.as_tensor(voice).numel() > 1:
            V = torch.as_tensor(voice).numel()
            rows1, _ = self._utterance_rows(what, codes, [0])
            rows, voices = self._utterance_rows(what, rows1 * V, voice)
            wavs, wav_bases = wavs * V, wav_bases * V
        else:
            rows, voices = self._utterance_rows(what, codes, voice)
        with torch.no_grad():
            self._check_codes(what, rows, eng.K)
            cuniq, code_bases, cat = {}, [], 0
            for r in rows:
                key = (r.data_ptr(), r.numel()) if r.numel() else ("empty", 0)
                if key not in cuniq:
                    cuniq[key] = (cat, r)
                    cat += r.numel()
                code_bases.append(cuniq[key][0])
            codes_flat = torch.cat([r.to(dev) for _, r in cuniq.values()]) if cat else torch.empty(0, dtype=torch.int64, device=dev)
            plan = CD.score_tile_plan([r.numel() for r in rows], [w.numel() for w in wavs], sg.plan_args(), eng.B)
            n_rows = len(rows)
            nll = torch.zeros(plan.n_total, dtype=torch.float32, device=dev)
            prob = torch.zeros(plan.n_total, dtype=torch.float32, device=dev) if return_prob else None
            hit = torch.zeros(plan.n_total, dtype=torch.uint8, device=dev) if return_hit else None
            # the summary's top-1 and mean probability need the two arrays whether the caller wants them or not
            prob_w = prob if prob is not None else torch.zeros(plan.n_total, dtype=torch.float32, device=dev)
            hit_w = hit if hit is not None else torch.zeros(plan.n_total, dtype=torch.uint8, device=dev)
            acc = torch.zeros(n_rows, 4, dtype=torch.float64, device=dev)
            out = torch.zeros(n_rows, 4, dtype=torch.float32, device=dev)
            if n_rows:
                eng.score_tiles(codes_flat, wav_flat, plan.table(code_bases, wav_bases, voices), nll, prob_w, hit_w,
                                offsets=plan.offsets, acc=acc, out=out)
        return CD.UtteranceScores(nll, torch.from_numpy(plan.offsets.copy()), out, acc, sg.o + sg.rf + 1, prob=prob, hit=hit,
                                  voice=torch.tensor(voices, dtype=torch.int64))

    # ---- comparing utterances: DTW over codebook rows and over the front-end's cepstra (align.py) ---------------------
    def code_distance(self, codes_a, codes_b=None, pairs=None, metric: str = "euclid", return_path: bool = False):
        """Dynamic time warping between code sequences, over their codebook rows: codes_a / codes_b a
        `codes.UtteranceCodes` or a list of 1-D int64 device tensors (codes_b=None: codes_a with itself), pairs (P, 2)
        indices into the two (default: zip) -> `align.Alignment` with device tensors cost, steps and mean = cost / steps,
        the distance inside ABX discrimination.  The rows of all sequences are looked up once (codes.lookup) into one
        ragged buffer that the alignment reads in place; metric / return_path as in align.dtw().  A code outside [0, K)
        raises AewError with the count before the alignment (the lookup never follows it; that check reads one word
        back).  VQ bottlenecks only.  The codebook is read, nothing of the model is written: no EMA statistic, histogram,
        loss or metric word; no collective under data parallel."""
        from . import align as AL
        sides, pr = self._code_sides("code_distance()", codes_a, codes_b, pairs)
        return AL.dtw(sides[0], None if codes_b is None else sides[1], pairs=pr, metric=metric, return_path=return_path)

    def _code_sides(self, what: str, codes_a, codes_b, pairs):
        """The front half of code_distance() / search_codes(): ([Ragged of the looked-up codebook rows per side], pairs);
        a code outside [0, K) raises before anything is compared."""
        from . import align as AL, codes as CD
        self._need_codes(what)
        if self._device.type != "cuda":
            raise L.AewError(f"{what} runs on an MI355X only; move the model to a cuda device first")
        rows_a = AL._symbol_rows(codes_a, f"{what}: codes_a")
        rows_b = None if codes_b is None else AL._symbol_rows(codes_b, f"{what}: codes_b")
        pr = AL.default_pairs(len(rows_a), None if rows_b is None else len(rows_b), pairs)
        with torch.no_grad():
            eng = self._engine if self._engine is not None else self._ensure_engine(int(self.hps.n_batch))
            self._dp_finish()
            emb = eng.emb.reshape(eng.K, -1)
            d = int(emb.shape[1])
            bad = torch.zeros(1, dtype=torch.int32, device=emb.device)
            sides = []
            for rows in (rows_a,) if rows_b is None else (rows_a, rows_b):
                lens = [int(r.numel()) for r in rows]
                base = [0]
                for n in lens:
                    base.append(base[-1] + n * d)
                zq = CD.lookup(emb, torch.cat([r.to(emb.device) for r in rows]), bad=bad)
                sides.append(AL.Ragged(zq.reshape(-1), base[:-1], lens, d, 1, d))
            n_bad = int(bad[0].item()) & 0xFFFFFFFF
            if n_bad:
                raise L.AewError(f"{what}: {n_bad} codes lie outside the codebook [0, {eng.K}); nothing was aligned")
            return sides, pr

    def cepstral_distance(self, wavs_a, wavs_b=None, pairs=None, expand: bool = True):
        """The mean DTW-aligned Euclidean distance between the cepstra of waveforms: wavs_a / wavs_b lists of 1-D device
        tensors of mu-law values, whole utterances of any lengths (wavs_b=None: wavs_a with itself), pairs as in
        align.dtw() -> `align.Alignment`; its `mean` is the distance, `cost` / `steps` what it is the quotient of.  The
        frames are the STATIC coefficients 1 .. n_mfcc - 1 of this model's own front-end (`DeviceMfcc.ragged`, one record
        per whole utterance): the energy coefficient 0 and the deltas are left out, and the channel-major arrays are
        read in place (chan_stride = frames).  expand=True turns the mu-law values into linear amplitudes first
        (codes.mu_decode) - the sound itself; expand=False feeds the mu-law values as the training front-end does.
        THE SCALE IS THIS FRONT-END'S - MFCC of dB power, orthonormal DCT - so the numbers are comparable between runs
        of this project and NOT with published mel-cepstral-distortion figures.  An utterance too short for
        `DeviceMfcc.MIN_FRAMES` frames has none: its pairs give inf.  VQ bottlenecks only (the rule of the utterance
        interface); nothing of the model is written and no collective is issued."""
        from . import align as AL
        sides = self._cepstral_sides("cepstral_distance()", wavs_a, wavs_b, expand)
        return AL.dtw(sides[0], None if wavs_b is None else sides[1], pairs=pairs, metric="euclid")

    def _cepstral_sides(self, what: str, wavs_a, wavs_b, expand: bool):
        """The front half of cepstral_distance() / search_wavs(): [Ragged of the static cepstra 1 .. n_mfcc - 1 per side],
        the channel-major arrays of `DeviceMfcc.ragged` read in place."""
        from . import align as AL, codes as CD
        self._need_codes(what)
        if self._device.type != "cuda":
            raise L.AewError(f"{what} runs on an MI355X only; move the model to a cuda device first")
        mf = self._utterance_mfcc()
        n_mfcc = int(mf.n_mfcc)
        if n_mfcc < 2:
            raise L.AewError(f"{what}: the front-end yields {n_mfcc} coefficient(s); none is left behind the energy term")
        sides = []
        with torch.no_grad():
            for wavs in (wavs_a,) if wavs_b is None else (wavs_a, wavs_b):
                wavs = list(wavs)
                for w in wavs:
                    if not torch.is_tensor(w) or w.dim() != 1:
                        raise L.AewError(f"{what}: lists of 1-D tensors of mu-law values expected")
                if expand:
                    wavs = [CD.mu_decode(w.to(self._device), int(self.n_quant)) for w in wavs]
                else:
                    wavs = [w.to(self._device) for w in wavs]
                flat, frames, bases = mf.ragged(wavs)
                sides.append(AL.Ragged(flat, [b + f for b, f in zip(bases, frames)], frames, 1, frames, n_mfcc - 1))
        return sides

    # ---- finding a query inside utterances: subsequence DTW over the same two feature sources (align.search) ----------
    def search_codes(self, query_codes, codes, pairs=None, metric: str = "euclid", n_hits: int = 1, rank: str = "mean",
                     min_len: int = 1, max_len: int = 0):
        """Where do the code sequences `query_codes` occur inside the code sequences `codes`: subsequence DTW over their
        codebook rows (align.search(); metric, n_hits, rank, min_len, max_len as there).  Both sides a
        `codes.UtteranceCodes` or a list of 1-D int64 device tensors, pairs (P, 2) = (query, document) indices (default:
        zip) -> `align.Matches`; start / end of a hit are CODE FRAMES of the document.  The front half is
        code_distance()'s: one lookup per side into a ragged buffer read in place, and a code outside [0, K) raises
        AewError before anything is searched.  VQ bottlenecks only; the codebook is read, nothing of the model is
        written and no collective is issued."""
        from . import align as AL
        sides, pr = self._code_sides("search_codes()", query_codes, codes, pairs)
        return AL.search(sides[0], sides[1], pairs=pr, metric=metric, n_hits=n_hits, rank=rank, min_len=min_len,
                         max_len=max_len)

    def search_wavs(self, query_wavs, wavs, pairs=None, expand: bool = True, n_hits: int = 1, rank: str = "mean",
                    min_len: int = 1, max_len: int = 0):
        """Where do the waveforms `query_wavs` occur inside the waveforms `wavs`: subsequence DTW (align.search(),
        Euclidean) over the static cepstra 1 .. n_mfcc - 1 of this model's own front-end - cepstral_distance()'s front
        half, `expand` as there.  Lists of 1-D device tensors of mu-law values, pairs (P, 2) = (query, document) indices
        (default: zip) -> `align.Matches`.  start / end of a hit are MFCC FRAMES of the document: consecutive frames lie
        `hop_sz` samples apart (160 by default) and each looks at `win_sz` samples (400), so a hit [start, end] covers
        about the samples start * hop_sz .. end * hop_sz + win_sz of the document.  Every utterance gets its own dB floor
        and delta edges, so a slice's cepstra are close to, not the bits of, the cepstra of the same samples inside a
        longer waveform.  A waveform too short for `DeviceMfcc.MIN_FRAMES` frames has none: its pairs find nothing.  VQ
        bottlenecks only; nothing of the model is written and no collective is issued."""
        from . import align as AL
        sides = self._cepstral_sides("search_wavs()", query_wavs, wavs, expand)
        return AL.search(sides[0], sides[1], pairs=pairs, metric="euclid", n_hits=n_hits, rank=rank, min_len=min_len,
                         max_len=max_len)

    # ---- discovering repeats between utterances: local-alignment DTW over the same two feature sources (align.discover) --
    def discover_codes(self, codes, codes_b=None, pairs=None, threshold: Optional[float] = None, metric: str = "euclid",
                       n_hits: int = 3, min_len: int = 1, max_len: int = 0, band: Optional[int] = None):
        """Which stretches of the code sequences `codes` repeat each other: local-alignment DTW over their codebook rows
        (align.discover(); threshold, metric, n_hits, min_len, max_len, band as there).  codes / codes_b a
        `codes.UtteranceCodes` or a list of 1-D int64 device tensors; codes_b=None compares `codes` with itself over
        every unordered pair including (u, u), pairs (P, 2) indices into the two -> `align.Repeats`; the starts and ends
        of a hit are CODE FRAMES.  The front half is code_distance()'s: one lookup per side into a ragged buffer read in
        place, and a code outside [0, K) raises AewError before anything is aligned.  VQ bottlenecks only; the codebook
        is read, nothing of the model is written and no collective is issued."""
        from . import align as AL
        if codes_b is None:
            pairs = AL.discover_pairs(len(codes), None, pairs)
        sides, pr = self._code_sides("discover_codes()", codes, codes_b, pairs)
        return AL.discover(sides[0], None if codes_b is None else sides[1], pairs=pr, threshold=threshold, metric=metric,
                           n_hits=n_hits, min_len=min_len, max_len=max_len, band=band)

    def discover_wavs(self, wavs, wavs_b=None, pairs=None, threshold: Optional[float] = None, expand: bool = True,
                      n_hits: int = 3, min_len: int = 1, max_len: int = 0, band: Optional[int] = None):
        """Which stretches of the waveforms `wavs` repeat each other: local-alignment DTW (align.discover(), Euclidean)
        over the static cepstra 1 .. n_mfcc - 1 of this model's own front-end - cepstral_distance()'s front half, `expand`
        as there, `threshold` on that front-end's scale.  Lists of 1-D device tensors of mu-law values; wavs_b=None
        compares `wavs` with itself over every unordered pair including (u, u) -> `align.Repeats`.  The starts and ends
        of a hit are MFCC FRAMES (see search_wavs() for what a frame covers).  A waveform too short for
        `DeviceMfcc.MIN_FRAMES` frames has none: its pairs find nothing.  VQ bottlenecks only; nothing of the model is
        written and no collective is issued."""
        from . import align as AL
        sides = self._cepstral_sides("discover_wavs()", wavs, wavs_b, expand)
        return AL.discover(sides[0], None if wavs_b is None else sides[1], pairs=pairs, threshold=threshold,
                           metric="euclid", n_hits=n_hits, min_len=min_len, max_len=max_len, band=band)

    # ---- ABX discriminability of a labelled item set over the same two feature sources (align.abx_task) ---------------
    def abx_codes(self, codes, category, speaker=None, mode: str = "within", metric: str = "euclid", value: str = "mean",
                  max_pairs: int = 1 << 20):
        """How well do the code sequences `codes` (a `codes.UtteranceCodes` or a list of 1-D int64 device tensors) keep
        their categories apart: the ABX error of the item set under DTW over the codebook rows.  category / speaker:
        one hashable label per item; mode "within" (A, B and X of one speaker), "across" (A and B of one speaker, X of
        another) or "any" (speakers ignored; speaker=None allowed).  All N (N - 1) / 2 distances are code_distance()'s
        (align.distance_matrix: metric, value "mean" = cost / steps or "cost", max_pairs pairs per launch), the triples
        are counted on the device (AEW_OP_ABX_COUNT) -> `align.AbxResult`: error (the mean over category pairs of the
        mean over speaker combinations), pooled, by_category, n_triples, all device tensors.  The rules of
        code_distance() apply: a code outside [0, K) raises AewError before anything is compared (that check reads one
        word back - the only wait); VQ bottlenecks only; the codebook is read, nothing of the model is written and no
        collective is issued."""
        from . import align as AL
        sides, _ = self._code_sides("abx_codes()", codes, None, None)
        return AL.abx_task(sides[0], category, speaker, mode=mode, metric=metric, value=value, max_pairs=max_pairs)

    def abx_wavs(self, wavs, category, speaker=None, mode: str = "within", expand: bool = True, value: str = "mean",
                 max_pairs: int = 1 << 20):
        """The ABX error of the waveforms `wavs` (a list of 1-D device tensors of mu-law values) under DTW over the static
        cepstra 1 .. n_mfcc - 1 of this model's own front-end - cepstral_distance()'s front half, `expand` as there,
        Euclidean frames; labels, mode, value, max_pairs and the result as in abx_codes().  It is the score of the
        model's INPUT features, the figure its codes are compared with.  A waveform too short for
        `DeviceMfcc.MIN_FRAMES` frames has no frames: its distances are +inf and every triple it enters counts as the
        order of +inf says.  VQ bottlenecks only; nothing of the model is written and no collective is issued."""
        from . import align as AL
        sides = self._cepstral_sides("abx_wavs()", wavs, None, expand)
        return AL.abx_task(sides[0], category, speaker, mode=mode, metric="euclid", value=value, max_pairs=max_pairs)

    def _grads_carried(self):
        """What the coming backward has to ADD to the gradients it writes: None when the gradients were cleared
        (FusedAdam.zero_grad(), or every .grad is None as zero_grad(set_to_none=True) leaves them), else a copy of the
        current values (zeros where a single .grad is None) - torch's accumulate-into-.grad rule."""
        eng = self._engine
        cleared, self._grads_cleared = self._grads_cleared, False
        if cleared:
            return None
        grads = [(name, self._parameters[pname].grad) for name, pname in self._pnames]
        if all(gr is None for _, gr in grads):
            return None
        if self._schedule.shards:
            raise L.AewError("backward() onto existing gradients (no zero_grad() since the last backward) is not supported "
                             "under the sharded data-parallel schedule: each rank holds the reduced gradient of its own "
                             "shards only")
        prev = eng.ps.grads[:eng.ps.numel].clone()
        for name, gr in grads:
            view = eng.ps.view(name, grad=True)
            o = (view.data_ptr() - eng.ps.grads.data_ptr()) // 4
            if gr is None:
                prev[o:o + view.numel()].zero_()
            elif gr.data_ptr() != view.data_ptr():               # somebody assigned their own tensor
                prev[o:o + view.numel()].copy_(gr.detach().reshape(-1).to(prev))
        return prev

    def _restart_codes(self, eng, min_usage: float, call: int):
        """One restart launch with the model's settings; through the data-parallel path where ranks have to agree."""
        kw = {k: (self._restart or _RESTART_DEFAULTS)[k] for k in _RESTART_DEFAULTS}
        self._schedule.restart_codes(eng, min_usage, call, **kw)

    def _auto_restart(self):
        """codebook_restart: the backward of step t = step_count + 1 restarts dead codes when t % every == 0, with call = t
        (step_count comes back from checkpoints: a resumed run restarts on the same steps with the same rows)."""
        opt = self._restart
        if opt is not None:
            t = self._engine.step_count + 1
            if t % opt["every"] == 0:
                self._restart_codes(self._engine, opt["min_usage"], t)

    def _after_backward(self, g, reduce=True):
        """reduce=False: a micro-batch inside an accumulated group - its gradient is not exchanged."""
        eng = self._engine
        self._fold_open = False
        # re-attach .grad views (optim.zero_grad(set_to_none=True) detaches them)
        for name, pname in self._pnames:
            self._parameters[pname].grad = eng.ps.view(name, grad=True)
        if reduce:
            self._schedule.reduce_grads(eng)
        # gradient statistics: AEW_OP_MOMENTS ops on a side lane of the backward plan (views, no kernels here)
        m = self.objective.metrics
        gs = eng.gstat
        if self.kind == "autoencoder":
            m["mel_grad_sd"], m["bn_grad_sd"] = gs[1], gs[5]
        else:
            m["mel_grad_sd"], m["mel_grad_mean"] = gs[1], gs[0]

    def _az_numel(self, eng):
        key = (eng.serial,)
        if getattr(self, "_az_cache", (None,))[0] != key:
            n = [eng.B * eng.geom.enc_lens[i + 1] * self.hps.enc_n_out for i in range(9)]
            self._az_cache = (key, torch.tensor(n, dtype=torch.float64, device=eng.enc.zero_cnt.device))
        return self._az_cache[1]

    def _fill_forward_metrics(self, eng):
        w, B = eng.n_win, eng.B
        n_pos = B * (w - 1)
        m = self.objective.metrics
        mb = eng.met_buf                                           # the "metrics" reduction op of the forward plan
        m["rec"] = mb[1]
        self.tprb_m = mb[2]                                        # chassis.py:266-270
        dg, pk = eng.diag, eng.diag_pk                             # AEW_OP_VQ_DIAG ops of the forward plan (side lanes)
        m["pk_m"], m["pk_sd"], m["pk_nuq"] = pk[6], pk[7], pk[8]    # vqema_bn.py:261-263
        if eng.bn is not None:                                      # the bottleneck type's own terms (engine.BottleneckPlan.metrics)
            m.update(eng.bn.metrics(mb, dg, eng.loss_buf))
        if self._restart is not None:
            m["vq_restarted"] = eng.restart_out()[1]                # codes the last restart re-seeded
        if eng.enc is not None and hasattr(self, "encoder"):
            az = eng.enc.zero_cnt[:9].double() / self._az_numel(eng)   # one division; the entries are views
            for i in range(9):
                self.encoder.metrics[f"enc_az_{i}"] = az[i]
