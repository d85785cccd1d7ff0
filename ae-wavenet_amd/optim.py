"""Fused Adam over the flat parameter buffer (one kernel launch for all 23.6 M parameters).

Numerically torch.optim.Adam with its defaults (the reference's optimizer, checkpoint.py:49-50).
Drop-in for the harness: `ss.optim = FusedAdam(model, lr)` in place of `t.optim.Adam(...)`.
"""
from __future__ import annotations

import contextlib
import fnmatch
import math

import numpy as np
import torch

from . import _lib as L
from .model import OptState

EMA_WARMUP_NUM, EMA_WARMUP_DEN = 1, 10       # decay of averaged step t with warm-up: min(ema_decay, (1 + t) / (10 + t))


def _check_ema_decay(d):
    if d is None:
        return None
    try:                                                     # like max_grad_norm: whatever float() takes (numpy scalars, 0-d tensors)
        f = float(d)
    except (TypeError, ValueError):
        f = float("nan")
    if not (0.0 < f < 1.0):
        raise ValueError(f"Invalid ema_decay: {d!r} (a number in (0, 1), or None for no averaged weights)")
    return f


def _check_max_grad_norm(c):
    if c is not None and not (float(c) > 0):
        raise ValueError(f"Invalid max_grad_norm: {c} (a positive number, or None for no clipping)")
    return c


def _check_flag(name, b):
    if not isinstance(b, (bool, int)) or b not in (0, 1):
        raise ValueError(f"Invalid {name}: {b!r} (True or False)")
    return bool(b)


def _check_rate(name, x):
    try:                                                     # whatever float() takes, like max_grad_norm
        f = float(x)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(x, bool) or not (math.isfinite(f) and f >= 0.0):
        raise ValueError(f"Invalid {name}: {x!r} (a finite number, not negative)")
    return f


def _check_frozen(b):
    if not isinstance(b, bool):
        raise ValueError(f"Invalid frozen: {b!r} (True or False)")
    return b


GROUP_KEYS = ("params", "lr", "weight_decay", "frozen")


def match_groups(names, groups):
    """groups = [dict(params=name | fnmatch pattern | list of them, lr=, weight_decay=, frozen=)] over the dotted parameter
    names -> [(indices into names, options)] per entry, in order: the first entry that matches a tensor takes it; the
    tensors no entry matches come last, with no options (the constructor's).  ValueError: an unknown key, no `params`, a
    pattern that matches no name at all, a rejected value."""
    taken, out = {}, []
    for k, entry in enumerate(groups):
        if not isinstance(entry, dict) or "params" not in entry:
            raise ValueError(f"groups[{k}]: a dict with a `params` key, got {entry!r}")
        for key in entry:
            if key not in GROUP_KEYS:
                raise ValueError(f"groups[{k}]: unknown key {key!r} (one of {GROUP_KEYS})")
        pats = entry["params"]
        pats = [pats] if isinstance(pats, str) else list(pats) if isinstance(pats, (list, tuple)) else []
        if not pats or not all(isinstance(p, str) for p in pats):
            raise ValueError(f"groups[{k}]: params must be a name, a pattern or a list of them, got {entry['params']!r}")
        opts = {}
        if "lr" in entry:
            opts["lr"] = _check_rate("lr", entry["lr"])
        if "weight_decay" in entry:
            opts["weight_decay"] = _check_rate("weight_decay", entry["weight_decay"])
        if "frozen" in entry:
            opts["frozen"] = _check_frozen(entry["frozen"])
        mine = []
        for pat in pats:
            hit = [i for i, n in enumerate(names) if fnmatch.fnmatchcase(n, pat)]
            if not hit:
                raise ValueError(f"groups[{k}]: pattern {pat!r} matches no parameter")
            for i in hit:
                if i not in taken:
                    taken[i] = k
                    mine.append(i)
        out.append((sorted(mine), opts))
    rest = [i for i in range(len(names)) if i not in taken]
    if rest:
        out.append((rest, {}))
    return out


def ema_decay_at(ema_decay: float, t: int, warmup: bool = True) -> float:
    """Decay of the averaged step number t (t = averaged steps taken before it), in double."""
    return min(float(ema_decay), (EMA_WARMUP_NUM + t) / (EMA_WARMUP_DEN + t)) if warmup else float(ema_decay)


def ema_rate_at(ema_decay: float, t: int, warmup: bool = True) -> float:
    """What the kernel multiplies by (aew_adam_t.avg_rate): 1 - decay in double, rounded to fp32 once."""
    return float(np.float32(1.0 - ema_decay_at(ema_decay, t, warmup)))


class FusedAdam(torch.optim.Optimizer):
    """The moments live in the engine's flat buffers (adam.m / adam.v, same offsets as the
    parameters); when no engine holds them (before the first run(), after model.to() / override() / a
    change of batch size) the model carries them (`HipModelBase._opt_carry`), so they survive every
    engine rebuild.  state_dict() / load_state_dict() speak torch.optim.Adam's format (per-parameter
    `step`, `exp_avg`, `exp_avg_sq`, parameters numbered in model.parameters() order) so that
    checkpoints interchange with the reference (checkpoint.py:61-63,87-98).

    max_grad_norm: clip the gradient to this global L2 norm inside the step - what
    `torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)` in front of `step()` does, as one launch over
    the flat gradient buffer whose result stays on the device (aew_grad_norm_t): the norm is that of
    grad_scale * gradient, after the data-parallel reduction; a step whose norm is inf / nan is skipped on the device
    (parameters and moments keep their bits, `skipped_steps` counts it; the step number still advances).  None = off.
    The value lives in `param_groups[0]["max_grad_norm"]`, where a schedule may change it.

    track_update_ratio: every step also leaves, per parameter tensor, the norm of its update, the norm of the weights
    before the step and their ratio on the device (`update_norm`, `weight_norm`, `update_ratio`) - what the reference's
    progress step computes with a clone of every parameter in front of `step()` and a loop of norms behind it
    (chassis.py:162-163,180-183), here summed inside the Adam launch (aew_uw_track_t): no clone, no host
    synchronisation, one summation order, and right under the sharded data-parallel schedule.  Parameters and moments
    are bit for bit those of an untracked step.  The value lives in `param_groups[0]["track_update_ratio"]`.

    ema_decay: every step also moves an exponential moving average of the parameters towards their new values inside
    the Adam launch (aew_adam_t.avg: avg += (1 - decay_t) * (p_new - avg), one more stream of that launch) - what a
    second copy of the parameters and a `torch._foreach_lerp_` behind `step()` do, and right under the sharded
    data-parallel schedule, where a rank owns its shards only at the moment of the update.  decay_t =
    min(ema_decay, (1 + t) / (10 + t)) for the averaged step t = 0, 1, ... with ema_warmup (the default), ema_decay
    without.  The average starts from the parameters in front of the first averaged step; a step the device skips leaves
    it alone.  Parameters and moments are bit for bit those of a step without it.  `averaged_weights()` puts the average
    in the parameters' place for sampling / evaluation.  A number in (0, 1), or None = off.  The values live in
    `param_groups[0]["ema_decay"]` / `["ema_warmup"]`.

    Gradient accumulation (`accumulate=k` on the model): inside a group - until the model's k-th backward - step() is a
    no-op: no launch, step count, moments, average and update-ratio record keep their bits.  Behind the k-th backward the
    gradient buffer holds the group's SUM and the step runs with grad_scale / k: the optimizer, the clip norm, the update
    ratios and the averaged weights see the MEAN of the micro-batch gradients - do not also divide the loss by k.  The
    state_dict gains no key.

    Parameter groups (`groups`, `weight_decay`, `requires_grad`): per-tensor learning rate, decoupled weight decay
    (torch.optim.AdamW: p *= 1 - lr * weight_decay in front of the Adam update) and frozen tensors, inside the same
    launch (aew_adam_groups_t) - so clipping, the update ratios, the averaged weights, accumulation and both data-parallel
    schedules go on working.  groups = [dict(params=name | fnmatch pattern | list of them, lr=, weight_decay=, frozen=)]
    over `model.named_parameters()`: the first entry that matches a tensor takes it, the tensors no entry matches form a
    last group with the constructor's lr / weight_decay.  `param_groups` is the torch list of these groups; step() reads
    every group's lr / weight_decay / frozen at each call, so torch.optim.lr_scheduler.* and hand-written schedules work
    per group.  `p.requires_grad_(False)` freezes a tensor too, with or without groups; it is read at each step().  A
    frozen tensor, its moments and its average keep their bits; the clip norm covers the trainable tensors only
    (clip_grad_norm_ over them).  betas, eps, max_grad_norm, track_update_ratio, ema_decay and ema_warmup stay optimizer-
    wide and are read from param_groups[0].  DEVIATIONS from torch: ONE step count for all tensors (a tensor unfrozen later
    continues with the global step and its old moments, where torch keeps a step per parameter and no state for a frozen
    one), and the backward still computes the gradients of frozen tensors (`.grad` shows them).  With no groups,
    weight_decay = 0 and nothing frozen the step is the launch of an optimizer without any of this, grid and bits, and
    state_dict() its dictionary key for key."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, max_grad_norm=None,
                 track_update_ratio=False, ema_decay=None, ema_warmup=True, weight_decay=0.0, groups=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, max_grad_norm=_check_max_grad_norm(max_grad_norm),
                        track_update_ratio=_check_flag("track_update_ratio", track_update_ratio),
                        ema_decay=_check_ema_decay(ema_decay), ema_warmup=_check_flag("ema_warmup", ema_warmup),
                        weight_decay=_check_rate("weight_decay", weight_decay), frozen=False)
        self.model = model
        named = list(model.named_parameters())
        self._index = {id(p): i for i, (_, p) in enumerate(named)}        # position in named_parameters() = ps.names() order
        if groups is None:
            super().__init__([p for _, p in named], defaults)
        else:
            _check_rate("lr", lr)
            super().__init__([dict(opts, params=[named[i][1] for i in idx])
                              for idx, opts in match_groups([n for n, _ in named], groups)], defaults)
        self.grad_scale = grad_scale

    def _tensor_records(self):
        """[(lr, weight_decay, frozen)] per tensor in named_parameters() order as the groups say NOW, or None where they
        say nothing a plain step does not do: one lr, no decay, nothing frozen."""
        plain, lr0 = True, self.param_groups[0]["lr"]
        if all(g["lr"] == lr0 and g.get("weight_decay", 0.0) == 0 and not g.get("frozen", False) for g in self.param_groups) \
                and all(p.requires_grad for g in self.param_groups for p in g["params"]):
            return None                                          # (the common case, kept short: it runs at every step)
        rec = [None] * len(self._index)
        for g in self.param_groups:
            lr, wd, fr = g["lr"], g.get("weight_decay", 0.0), g.get("frozen", False)
            for p in g["params"]:
                f = bool(fr) or not p.requires_grad
                rec[self._index[id(p)]] = (lr, wd, f)
                plain = plain and not f
            plain = plain and wd == 0 and lr == lr0
        if plain:
            return None
        for g in self.param_groups:                              # (a schedule may have put anything there)
            _check_rate("lr", g["lr"]); _check_rate("weight_decay", g.get("weight_decay", 0.0))
            _check_frozen(g.get("frozen", False))
        if any(r is None for r in rec):
            raise ValueError("param_groups no longer hold every parameter of the model")
        return [(float(lr), float(wd), f) for lr, wd, f in rec]

    def _grouped(self):
        """Does the state dictionary need more than one plain group?"""
        return len(self.param_groups) > 1 or any(g.get("weight_decay", 0.0) != 0 or g.get("frozen", False)
                                                 for g in self.param_groups)

    @torch.no_grad()
    def step(self, closure=None):
        eng = self.model._engine
        if eng is None:
            raise RuntimeError("FusedAdam.step() before the first model.run()")
        g = self.param_groups[0]
        c = _check_max_grad_norm(g.get("max_grad_norm"))
        track = bool(g.get("track_update_ratio"))
        d = _check_ema_decay(g.get("ema_decay"))
        if eng.averaged_in:
            raise L.AewError("FusedAdam.step() inside averaged_weights(): the averaged weights sit in the parameters' place")
        k = getattr(self.model, "accumulate", 1)
        scale = self.grad_scale
        if k > 1:
            # gradient accumulation: a step inside a group is a no-op (no launch, no counter moves); the step behind the
            # group's k-th backward sees the SUM in the gradient buffer and takes the mean through the scale
            if not self.model.group_ready:
                return
            scale = self.grad_scale / k                          # (in double; rounded to fp32 where grad_scale is)
            self.model._group_ready = False
        kw = {}
        if d is not None:                                        # (off: the calls below are the ones of an optimizer without it)
            kw["avg_rate"] = ema_rate_at(d, eng.avg_steps, bool(g.get("ema_warmup", True)))
        rec = self._tensor_records()
        if rec is not None:                                      # (plain: the calls below are the ones of an optimizer without groups)
            kw["groups"] = rec
        # (data parallel, sharded: Adam on this rank's shards of the reduce-scattered gradient, then all-gather)
        self.model._schedule.step(eng, g["lr"], scale, betas=g["betas"], eps=g["eps"], max_grad_norm=c, track=track, **kw)

    # ---- the averaged weights -------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block the model computes with the averaged weights: `model.sample`, `model.forward`, `model.run` and
        `model.state_dict()` see them (one swap launch on the device; the sampler re-packs); `step()`, `load_state_dict()`,
        `model.to()` and `model.override()` raise.  On exit - also by an exception - the swap is undone: parameters and
        average are bit for bit what they were."""
        model = self.model
        # (whether the average is swapped in is the engine's to say: inside the block an engine may change, not go away)
        if model._engine is not None and model._engine.averaged_in:
            raise L.AewError("averaged_weights() is already entered")
        st = model._opt_state(avg=True)                          # (raises where this rank's average is incomplete: sharded DP)
        if st is None or st.avg_steps < 1:
            raise L.AewError("averaged_weights(): no averaged step has run yet (FusedAdam(..., ema_decay=...) and step())")
        model._dp_finish()                                       # parameter all-gathers in flight write what the swap reads
        # the swap is a launch on the engine's buffers: with none live (a restored checkpoint, model.to()) the sampling
        # engine is built, which takes the carried average in
        (model._engine or model._ensure_engine(1)).swap_averaged()
        try:
            yield self
        finally:
            model._engine.swap_averaged()                        # (sample() inside may have moved everything to the B = 1
                                                                 #  engine; to() / override() are refused while swapped in)

    # ---- what the last clipped step saw (0-d device tensors: reading one is the caller's synchronisation) ----------
    def _clip_word(self, i):
        eng = self.model._engine
        if eng is None:
            raise RuntimeError("FusedAdam: no step has run yet")
        return eng.grad_norm()[i]

    @property
    def grad_norm(self):
        """Global norm of grad_scale * gradient at the last step taken with max_grad_norm (before clipping)."""
        return self._clip_word(0)

    @property
    def clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of that step; 0 when its norm was inf / nan."""
        return self._clip_word(1)

    @property
    def skipped_steps(self):
        """Steps skipped so far because their gradient norm was inf / nan (counted on the device)."""
        return self._clip_word(3)

    # ---- what the last tracked step did per tensor ({parameter name: 0-d device tensor}, named_parameters() order) ---
    def _ratio_row(self, i):
        eng = self.model._engine
        if eng is None:
            raise RuntimeError("FusedAdam: no step has run yet")
        out = eng.update_ratios()                                # [3][P] views; P in the flat buffer's = named_parameters() order
        return {name: out[i, k] for k, (name, _) in enumerate(self.model.named_parameters())}

    @property
    def update_norm(self):
        """||p_before - p_after|| per parameter tensor at the last step taken with track_update_ratio (0 for a step the
        device skipped)."""
        return self._ratio_row(0)

    @property
    def weight_norm(self):
        """||p_before|| per parameter tensor of that step."""
        return self._ratio_row(1)

    @property
    def update_ratio(self):
        """update_norm / weight_norm, a plain fp32 division: inf / nan for a zero-initialised tensor, as the reference's
        `t.norm(c - p.data) / c.norm()`."""
        return self._ratio_row(2)

    # ---- torch.optim.Adam-compatible state -------------------------------------------------
    def _layout(self):
        """[(name, flat offset, numel, shape)] and the flat length: the ParamStore rule (engine.py), computed from
        the parameter specs so that it is known without an engine."""
        out, o = [], 0
        for name, p in self.model.named_parameters():
            k = p.numel()
            out.append((name, o, k, tuple(p.shape)))
            o += (k + 3) // 4 * 4
        return out, o

    def state_dict(self):
        lay, _ = self._layout()
        g = self.param_groups[0]
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(lay)))}
        if g.get("max_grad_norm") is not None:                  # (an extra key: torch.optim.Adam.load_state_dict carries it along)
            group["max_grad_norm"] = g["max_grad_norm"]
        if g.get("track_update_ratio"):
            group["track_update_ratio"] = True
        av = None
        if g.get("ema_decay") is not None:                      # (off: the dictionary is the one of an optimizer without it)
            av = self.model._opt_state(avg=True)
            group["ema_decay"], group["ema_warmup"] = g["ema_decay"], bool(g.get("ema_warmup", True))
            group["avg_steps"] = av.avg_steps if av is not None else 0
        state = {}
        st = self.model._opt_state()
        if st is not None and st.step > 0:
            m, v = st.m.detach().cpu(), st.v.detach().cpu()     # (synchronises with the stream that wrote them)
            for i, (n, o, k, shp) in enumerate(lay):
                state[i] = {"step": torch.tensor(float(st.step)), "exp_avg": m[o:o + k].reshape(shp).clone(),
                            "exp_avg_sq": v[o:o + k].reshape(shp).clone()}
            if av is not None and av.avg_steps > 0:
                a = av.avg.detach().cpu()
                for i, (n, o, k, shp) in enumerate(lay):
                    state[i]["param_avg"] = a[o:o + k].reshape(shp).clone()
        if not self._grouped():
            return {"state": state, "param_groups": [group]}
        # several groups: torch's format - `params` holds the tensors' positions in model.parameters() order (what a
        # one-group file numbers them by), every group its lr / weight_decay, `frozen` where set; the optimizer-wide
        # extras stay in group 0.  A stock torch.optim.AdamW built with the same grouping loads it.
        decays = any(gg.get("weight_decay", 0.0) != 0 for gg in self.param_groups)
        out = []
        for k, gg in enumerate(self.param_groups):
            one = dict(group) if k == 0 else {key: group[key] for key in ("betas", "eps", "amsgrad", "maximize", "foreach",
                                                                           "capturable", "differentiable", "fused")}
            one["lr"], one["weight_decay"] = gg["lr"], gg.get("weight_decay", 0.0)
            one["params"] = [self._index[id(p)] for p in gg["params"]]
            if gg.get("frozen", False):
                one["frozen"] = True
            if decays:
                one["decoupled_weight_decay"] = True
            out.append(one)
        return {"state": state, "param_groups": out}

    def load_state_dict(self, state_dict):
        if self.model._engine is not None and self.model._engine.averaged_in:
            raise L.AewError("load_state_dict() inside averaged_weights()")     # (before anything is changed)
        lay, total = self._layout()
        groups = state_dict["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if len(order) != len(lay):
            raise ValueError(f"optimizer state has {len(order)} parameters, the model {len(lay)}")
        g0 = groups[0]
        # per-group options: a file with one group leaves them as the constructor set them (its lr is taken where this
        # optimizer has one group too); a file with several must cut the parameters the way this optimizer does
        mine = [[self._index[id(p)] for p in g["params"]] for g in self.param_groups]
        per_group = []
        if len(groups) > 1:
            if sorted(order) != list(range(len(lay))):
                raise ValueError(f"optimizer state with {len(groups)} groups must number the parameters 0..{len(lay) - 1} once each")
            by_set = {frozenset(idx): k for k, idx in enumerate(mine)}
            for k, g in enumerate(groups):
                hit = by_set.get(frozenset(g["params"]))
                if hit is None or len(groups) != len(mine):
                    names = [lay[i][0] for i in g["params"][:3]]
                    raise ValueError(f"optimizer state: group {k} of the file ({len(g['params'])} parameters: {names} ...) is "
                                     f"no group of this optimizer ({len(mine)} groups, the file {len(groups)})")
                o = {"frozen": _check_frozen(bool(g.get("frozen", False)))}
                if "lr" in g:
                    o["lr"] = _check_rate("lr", g["lr"])
                if "weight_decay" in g:
                    o["weight_decay"] = _check_rate("weight_decay", g["weight_decay"])
                per_group.append((hit, o))
        # the optimizer-wide options; one that is absent (a torch.optim.Adam checkpoint) keeps the constructor's
        opts = {k: tuple(g0[k]) if k == "betas" else g0[k] for k in (("lr", "betas", "eps") if len(mine) == 1 else ("betas", "eps"))
                if k in g0}
        if g0.get("max_grad_norm") is not None:
            opts["max_grad_norm"] = g0["max_grad_norm"]
        if g0.get("track_update_ratio") is not None:
            opts["track_update_ratio"] = bool(g0["track_update_ratio"])
        if g0.get("ema_decay") is not None:
            opts["ema_decay"], opts["ema_warmup"] = _check_ema_decay(g0["ema_decay"]), bool(g0.get("ema_warmup", True))
        st = state_dict.get("state", {})
        m, v = torch.zeros(total), torch.zeros(total)
        avg, n_avg = torch.zeros(total), 0
        step, found = 0, False
        for pos, idx in enumerate(order):
            s = st.get(idx, st.get(str(idx)))
            if s is None:
                continue
            n, o, k, shp = lay[idx if len(groups) > 1 else pos]
            if tuple(s["exp_avg"].shape) != shp:
                raise ValueError(f"exp_avg of parameter {n} has shape {tuple(s['exp_avg'].shape)}, expected {shp}")
            m[o:o + k] = s["exp_avg"].detach().float().cpu().reshape(-1)
            v[o:o + k] = s["exp_avg_sq"].detach().float().cpu().reshape(-1)
            step = max(step, int(float(s["step"])))
            found = True
            if s.get("param_avg") is not None:
                if tuple(s["param_avg"].shape) != shp:
                    raise ValueError(f"param_avg of parameter {n} has shape {tuple(s['param_avg'].shape)}, expected {shp}")
                avg[o:o + k] = s["param_avg"].detach().float().cpu().reshape(-1)
                n_avg += 1
        if n_avg not in (0, len(order)):
            raise ValueError(f"optimizer state has param_avg for {n_avg} of {len(order)} parameters")
        self.param_groups[0].update(opts)                        # every check has passed by here
        for hit, o in per_group:
            self.param_groups[hit].update(o)
        if not found:
            return
        # the averaged weights: restored with their step count; a state without them (torch.optim.Adam's own, or written
        # before the first averaged step) leaves none - the average then starts from the parameters at the next step
        self.model._load_opt_state(OptState(step, m, v, max(1, int(g0.get("avg_steps", step))), avg) if n_avg
                                   else OptState(step, m, v))

    def zero_grad(self, set_to_none=True):
        # the backward plan rewrites the flat gradient buffer: "cleared" is a flag the next backward reads (no memset;
        # without it the next backward adds to the existing .grad like any torch module, surface._grads_carried)
        self.model._grads_cleared = True
        if set_to_none:
            # like torch: nothing that looks at .grad between zero_grad() and the next backward sees last step's values
            # (the backward re-attaches the views into the flat gradient buffer, surface._after_backward)
            for p in self.model.parameters():
                p.grad = None
        else:
            # torch's set_to_none=False contract: .grad reads as zeros right away (the views point into the flat gradient
            # buffer, which the next backward rewrites anyway: one 95 MB fill, ~15 us)
            eng = getattr(self.model, "_engine", None)
            if eng is not None:
                eng.ps.grads[:eng.ps.numel].zero_()
        return None
