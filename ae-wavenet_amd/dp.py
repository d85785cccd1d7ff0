"""Data parallelism: one process per GPU, RCCL over xGMI via torch.distributed.

The reference only distributes on TPU (xmp.spawn + xm.optimizer_step, train.py:58-60,
chassis.py:168-169).  Here every rank holds a full replica and an independent shard of audio
windows (sampler rule data.py:100-106); per step the ranks exchange
  * the gradients (SUM; the optimizer applies 1/world for mean-type losses — SURVEY §8e), and
  * the VQ-EMA statistics z_sum / n_sum (SUM) before the EMA update, so that all replicas keep
    an identical codebook (north-star requirement; the reference lets replicas drift).

A step through the module surface (model.run, loss.backward, FusedAdam.step) runs under ONE schedule object - LocalSchedule
(nothing attached, or one rank without force_collectives), AllReduceSchedule (dp.attach(model)) or ShardedSchedule
(dp.attach(model, sharded=True)) - picked by DataParallel.schedule() at every use (HipModelBase._schedule).  Its interface is
all that surface.py, optim.py and grad_analysis.py know of a schedule; the table of who does what is in DESIGN.md §6.

Two schedules for the gradient exchange (same result up to fp32 summation order):
  train_step          all-reduce of the decoder tail under the encoder backward, all-reduce of the head under the
                      decoder's Adam range (round 1);
  train_step_sharded  reduce-scatter + SHARDED Adam + all-gather (what xm.optimizer_step amounts to on a ring):
                      every rank receives and updates only its 1/world shard of each region (a ring reduce-scatter moves
                      half the bytes of an all-reduce before the optimizer can start, and the Adam pass shrinks by
                      world), then the updated shards are all-gathered; the decoder region's reduce-scatter runs under the
                      encoder backward, and its all-gather - issued behind the head's - under the NEXT step's encoder
                      forward: forward() waits for the head's parameters before the first forward plan and for the
                      decoder's only between the two (TrainEngine.pack_dec_late).  Optional
                      bf16 gradient transport (half the xGMI bytes of the reduce-scatter; fp32 master parameters and
                      moments unchanged).

Gradient clipping (max_grad_norm in the Adam keywords; aew_grad_norm_t): the coefficient needs the norm of the WHOLE reduced
gradient, so in such a step no Adam range runs before every region is reduced - the overlap of the decoder's Adam with
the encoder's reduction is given up.  All-reduce schedule: every rank holds the full reduced gradient and computes the
same norm, no collective.  Sharded schedule: a rank holds reduced values only for its shards and the replicated
remainders; it sums its shards, the ranks all-reduce that ONE fp64 word, and a second launch adds the remainders (equal
on every rank, so counted once).  torch.nn.utils.clip_grad_norm_ on the .grad views must NOT be used with the sharded
schedule: after loss.backward() the reduce-scatters are still in flight and .grad holds this rank's unreduced values.

Update / weight ratios (track in the Adam keywords; aew_uw_track_t): the Adam launches sum per chunk of the parameter
tensors they cover.  All-reduce schedule: every rank updates everything - the two range calls of train_step leave the
sums of a whole-buffer step, no collective.  Sharded schedule: every rank sums over its shards, rank 0 alone over the
replicated remainders (equal on every rank: counted once); the per-tensor fp64 pairs are all-reduced (2 P words) and a
finalizing launch takes norms and ratios from them, so every rank holds the same ratios while the parameter all-gathers
are still in flight.  The reference's clone-and-norm loop around optim.step() must NOT be used with the sharded schedule:
after the step p.data is complete only once those all-gathers are.

Averaged weights (avg_rate in the Adam keywords; aew_adam_t.avg): the Adam launch averages the elements it updates.
All-reduce schedule: every rank runs the same whole-buffer step, nothing else to do.  Sharded schedule: a rank averages
its own shards and the replicated remainders - like the moments, its average is complete for its own shards only until
gather_moments() / sync_optimizer_state() all-gathers adam_avg along with them; FusedAdam.averaged_weights() refuses to
swap in an incomplete average.  A copy of the parameters updated with torch._foreach_lerp_ behind optim.step() must NOT
be used with the sharded schedule: p.data is complete only once the parameter all-gathers are.

Gradient accumulation (`accumulate=k` on the model; aew_accum_t): the micro-batches 1 .. k-1 of a group exchange nothing -
no gradient collective, no EMA-statistics collective (the VAE's KL all-reduce belongs to a micro-batch's own backward and
stays).  The k-th micro-batch exchanges the group's sums, as often per group as a step does without accumulation.
All-reduce schedule: allreduce_grads behind the fold that leaves the sum in the gradient buffer.  Sharded schedule:
backward_exchange(accum_last=True) folds each region in front of its reduce-scatter, so the overlap with the encoder
backward is kept.  The statistics all-reduce (sync or async, finish_ema unchanged) runs on the group's z_sum / n_sum; the
parameter all-gathers follow real optimizer steps only.

Parameter groups (groups in the Adam keywords; aew_adam_groups_t): every range / shard / remainder call of a step carries
the per-tensor records, so a tensor is stepped with its own rate and decay, or left alone, wherever a shard cut falls.  The
clip norm covers the trainable tensors only.  All-reduce schedule: the first range call takes it over their element
ranges, no collective.  Sharded schedule: a rank's shards and the replicated remainders are cut to those ranges
(TrainEngine.trainable_ranges; more than 8: chained launches) - the ONE fp64 word and the second launch are unchanged.
The gradients of frozen tensors are still exchanged: the backward plan does not know about them.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.distributed as dist

from . import _lib as L


def shard_indices(n: int, rank: int, world: int, epoch: int) -> List[int]:
    """Replica-sharded looping sampler order of the reference (data.py:100-106)."""
    g = torch.Generator()
    g.manual_seed(epoch * world + rank)
    vals = list(range(rank, n, world))
    perm = torch.randperm(len(vals), generator=g).tolist()
    return [vals[i] for i in perm]


class LocalSchedule:
    """A step that exchanges nothing.  The interface of all three schedules; fold: None, or the AEW_OP_ACCUM mode of this
    micro-batch in a group of accumulated ones (collectives and codebook upkeep run with a group's LAST one only)."""
    shards = False                          # True: .grad holds reduced values for this rank's shards only

    def _nothing(self, *args):
        pass

    wait_params = _nothing                  # (): in front of a run() - the parameters its forward reads are complete
    wait_all = _nothing                     # (): in front of every other reader of the parameters - no all-gather in flight
    reduce_grads = _nothing                 # (eng): behind the backward AND the code restart of a step / a group's last fold
    abandon = _nothing                      # (): an exchange no optimizer step will complete (a finished group dropped)

    def forward(self, eng, ema_allreduce, fold=None):
        return eng.forward(ema_allreduce, **({} if fold is None else {"accum": fold}))

    def backward(self, eng, fold=None):     # the ONE backward path: the plan writes the micro-batch's gradient, then the fold
        eng.backward(**({} if fold is None else {"refresh_codebook": fold == L.ACCUM_LAST}))
        if fold is not None:
            eng.accum_grads(fold)           # (FIRST, ADD ..., and LAST, which leaves the group's SUM in .grad)

    def step(self, eng, lr, grad_scale, **adam_kw):
        eng.adam_step(lr, grad_scale, **adam_kw)

    def restart_codes(self, eng, min_usage, call, **kw):
        eng.restart_codes(min_usage, call, **kw)

    def eval_finish(self, eng):
        return eng.eval_finish()

    def eval_group_finish(self, eng):
        gout, tout = eng.eval_group_finish()
        return gout.clone(), tout.clone()


class AllReduceSchedule(LocalSchedule):
    """The backward leaves the fully reduced gradient in every .grad, every rank runs the whole Adam step.  The
    DataParallel's methods are looked up when they are called (tests and tools wrap them on the instance)."""

    def __init__(self, dp):
        self.dp = dp

    def wait_all(self):
        self.dp.finish()

    wait_params = wait_all                  # (the parameter all-gathers of a preceding sharded step)

    def backward(self, eng, fold=None):
        self.dp.allreduce_kl(eng)           # VAE: the clamp's gate sees the global KL (every micro-batch's own)
        super().backward(eng, fold)

    def reduce_grads(self, eng):
        self.dp.allreduce_grads(eng)

    def restart_codes(self, eng, min_usage, call, **kw):
        self.dp.restart_codes(eng, min_usage, call, **kw)

    def eval_finish(self, eng):
        return self.dp.eval_finish(eng)

    def eval_group_finish(self, eng):
        return self.dp.eval_group_finish(eng)


class ShardedSchedule(AllReduceSchedule):
    """Reduce-scatter under the backward, sharded Adam, all-gather (forward / backward_exchange / optimizer_step below)."""
    shards = True
    wait_params = reduce_grads = LocalSchedule._nothing      # (forward() waits for the parameters region by region)

    def forward(self, eng, ema_allreduce, fold=None):       # (the statistics go through dp.allreduce_ema_async)
        return self.dp.forward(eng, **({} if fold is None else {"accum": fold}))

    def backward(self, eng, fold=None):
        if fold in (L.ACCUM_FIRST, L.ACCUM_ADD):             # inside a group nothing is exchanged
            return super().backward(eng, fold)
        # reduce-scatter issued under the encoder backward; a group's last micro-batch: each region's LAST fold in front of it
        self.dp.backward_exchange(eng, self.dp.bf16_grads, **({} if fold is None else {"accum_last": True}))

    def step(self, eng, lr, grad_scale, **adam_kw):
        self.dp.optimizer_step(eng, lr, grad_scale, **adam_kw)

    def abandon(self):
        self.dp.abandon_exchange()


class DataParallel:
    def __init__(self, bucket_mb: float = 32.0, group=None, force_collectives: bool = False):
        """force_collectives: issue every collective also in a process group of ONE rank (they are identities there).  A
        one-GPU box can then put RCCL under the product's exact calls - views, dtypes, stream ordering against graph
        replays - which the world == 1 short cuts below would otherwise skip (tests/test_dp_gpu.py)."""
        if not dist.is_initialized():
            raise RuntimeError("torch.distributed is not initialised")
        self.group = group
        self.force_collectives = bool(force_collectives)
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.bucket_elems = int(bucket_mb * (1 << 20) // 4)
        self.sharded, self.bf16_grads = False, False
        self._pending, self._st = [], None
        self._bufs = {}                     # persistent transport buffers by (kind, region start, elements, dtype)
        self.moments_step = -1              # engine step count for which every rank holds ALL Adam moments
        self.timing = False                 # True: bracket every wait with events (exposed_ms())
        self._tev = []

    def _solo(self) -> bool:
        """One rank and no request to run the collectives anyway: every exchange is skipped."""
        return self.world == 1 and not self.force_collectives

    def schedule(self):
        """The exchange schedule of a step through the module surface, for the state this object is in NOW."""
        return LocalSchedule() if self._solo() else ShardedSchedule(self) if self.sharded else AllReduceSchedule(self)

    # ---- measurement: how long the compute stream actually stalls on collectives ---------------------------------
    def _wait(self, work, what: str):
        """work.wait() - with `timing` on, bracketed by events on the current stream: the elapsed time between them is
        the part of the collective that was NOT hidden under compute (nothing else runs between the two records)."""
        if not self.timing or not torch.cuda.is_available():
            work.wait()
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        work.wait()
        e1.record()
        self._tev.append((what, e0, e1))

    def exposed_ms(self, reset: bool = True):
        """{wait point: total exposed ms since the last reset} (synchronises)."""
        out = {}
        if self._tev:
            torch.cuda.synchronize()
            for what, e0, e1 in self._tev:
                out[what] = out.get(what, 0.0) + e0.elapsed_time(e1)
        if reset:
            self._tev = []
        return out

    def _buf(self, kind: str, start: int, numel: int, dtype, device) -> torch.Tensor:
        key = (kind, start, numel, dtype)
        t = self._bufs.get(key)
        if t is None or t.device != device:
            t = torch.empty(numel, dtype=dtype, device=device)
            self._bufs[key] = t
        return t

    # ---- the chained launches' sticky timeout word (TrainEngine.chain_guard) --------------------------------------------
    def _guard_sync(self, eng):
        """A hand-off wait that gave up on ONE rank poisons that rank's gradients - and through the exchange everybody's.
        The guard word the Adam / EMA ops read is therefore MAX-reduced over the ranks in front of the first gradient
        collective of a step (4 bytes, asynchronous, completes before the gradients do: same communicator, issue order),
        so every rank skips the update of such a step, not only the one that saw the timeout."""
        if self._solo() or getattr(eng, "chain_guard", None) is None or not eng._chain_flags():
            return
        self._guard_work = dist.all_reduce(eng.chain_guard[:1], op=dist.ReduceOp.MAX, group=self.group, async_op=True)

    def _guard_wait(self):
        w, self._guard_work = getattr(self, "_guard_work", None), None
        if w is not None:
            self._wait(w, "chain.guard")

    def _warn_merged_packs(self, eng):
        """TrainEngine.merge_packs = None resolves at engine construction from the torch.distributed state; an engine built
        BEFORE init_process_group packs every weight layout at the head of the first forward plan, and the decoder's
        parameter all-gather can then not stay in flight under the encoder forward (_late() is False).  Results are the
        same; the overlap is lost - say so once."""
        if self.world > 1 and self.sharded and getattr(eng, "merge_packs", False) and getattr(eng, "merge_packs_auto", False) \
                and not getattr(self, "_warned_packs", False):
            import warnings
            self._warned_packs = True
            warnings.warn("ae_wavenet_amd.dp: the engine was built before torch.distributed was initialised, so it packs all weight "
                          "layouts in ONE launch at the head of the forward (TrainEngine.merge_packs); the decoder's parameter "
                          "all-gather is then not overlapped with the encoder forward.  Build the model after "
                          "init_process_group, or set TrainEngine.merge_packs = False.")

    def grad_scale(self, mean_loss: bool) -> float:
        """Factor the optimizer applies to the summed gradient: 1/world reproduces the
        single-process gradient of a mean-type loss over the global batch; sum-type losses
        (VQ) keep the sum.  The VAE mixes both (mean NLL + annealed, clamped SUM of KL, vae_bn.py:90-125):
        prepare_vae() makes its KL part come out right under the 1/world factor."""
        return 1.0 / self.world if mean_loss else 1.0

    def prepare_vae(self, eng):
        """VAE under data parallel = the single-process objective over the global batch:
        mean(NLL over all ranks' positions) + anneal * clamp(sum of KL over ALL ranks' windows, min=free_nats).
        (1) the KL gradient coefficient is pre-multiplied by world (the optimizer divides the summed gradient by
        world for the mean-type NLL); (2) the free-nats gate of the clamp must see the GLOBAL KL: allreduce_kl()
        between forward and backward."""
        if eng.bn_type == "vae":
            eng.dp_world = self.world
            eng.set_anneal_weight(eng.anneal_weight)

    def allreduce_kl(self, eng):
        """Sum the KL value the backward's clamp gate reads (loss_buf[2]) over the ranks (VAE only)."""
        if eng.bn_type == "vae" and not self._solo():
            dist.all_reduce(eng.loss_buf[2:3], op=dist.ReduceOp.SUM, group=self.group)

    def allreduce_grads(self, eng):
        flat = eng.ps.grads[:eng.ps.numel]
        if self._solo():
            return
        self._guard_sync(eng)
        self._guard_wait()
        n = flat.numel()
        for s in range(0, n, self.bucket_elems):
            dist.all_reduce(flat[s:s + self.bucket_elems], op=dist.ReduceOp.SUM, group=self.group)

    def backward_allreduce(self, eng):
        """Backward with the gradient exchange overlapped.  The flat gradient buffer is
        [encoder | bottleneck | decoder]; the decoder part (~40 % of the bytes at arch.vqvae-ema) is final
        once the decoder backward and its unpack are done, so its all-reduce is issued there
        (async, on the collective's own stream) and runs under the bottleneck / encoder backward.
        The head of the buffer follows when the backward is complete.  Numerically identical to
        backward() + allreduce_grads()."""
        if self._solo():
            eng.backward()
            return
        n, lo = eng.ps.numel, eng.dec_grad_offset
        flat = eng.ps.grads
        work = []

        def after_decoder():
            self._guard_sync(eng)
            work.append(dist.all_reduce(flat[lo:n], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

        eng.backward(after_decoder=after_decoder)
        if lo > 0:
            work.append(dist.all_reduce(flat[:lo], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        self._guard_wait()
        for w in work:
            w.wait()

    def train_step(self, eng, lr: float, grad_scale: float = 1.0, **adam_kw):
        """forward + backward + Adam with every collective off the critical path that can be:
          * EMA statistics: async all-reduce issued after the encoder / VQ part of the forward, consumed by the
            (deferred) EMA accumulation after the backward;
          * decoder gradients: async all-reduce between the two backward plans (under the encoder backward);
          * encoder gradients: all-reduce after the backward, under the Adam update of the decoder range.
        With max_grad_norm (an Adam keyword) both reductions are waited for first: the norm launch reads the whole
        reduced buffer (identical on every rank, so no collective), then the two Adam ranges run."""
        if self._solo():
            eng.forward()
            eng.backward()
            eng.adam_step(lr, grad_scale, **adam_kw)
            return
        n, lo = eng.ps.numel, eng.dec_grad_offset
        flat = eng.ps.grads
        work = {}
        self.finish()                       # parameter all-gathers of a preceding sharded step

        def after_decoder():
            self._guard_sync(eng)
            work["dec"] = dist.all_reduce(flat[lo:n], op=dist.ReduceOp.SUM, group=self.group, async_op=True)

        eng.forward(self.allreduce_ema_async)
        self.allreduce_kl(eng)
        eng.backward(after_decoder=after_decoder)
        if lo > 0:
            work["enc"] = dist.all_reduce(flat[:lo], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        self._guard_wait()
        self._wait(work["dec"], "grads.decoder")
        if lo > 0 and adam_kw.get("max_grad_norm") is not None:
            self._wait(work.pop("enc"), "grads.encoder")         # the norm (first range, count=True) reads every gradient
        eng.adam_step(lr, grad_scale, lo=lo, hi=n, **adam_kw)
        if lo > 0:
            if "enc" in work:
                self._wait(work["enc"], "grads.encoder")
            eng.adam_step(lr, grad_scale, lo=0, hi=lo, count=False, **adam_kw)
        self.moments_complete_at(eng.step_count)    # all-reduce schedule: every rank updates everything

    # ---- reduce-scatter + sharded Adam + all-gather ------------------------------------------------------------
    def _split(self, a: int, b: int):
        """Region [a, b) of the flat buffer -> (shard elements s, remainder start): world * s elements are reduce-
        scattered (rank r owns [a + r*s, a + (r+1)*s)), the < 4*world elements from the remainder start are all-reduced
        and updated by every rank.  s is a multiple of 4 (the Adam kernel works on float4)."""
        s = ((b - a) // (4 * self.world)) * 4
        return s, a + self.world * s

    def _reduce_region(self, flat: torch.Tensor, a: int, b: int, bf16: bool):
        """Issue the reduction of gradient region [a, b): returns a list of async work handles and a `finish`
        callable to run after they completed (bf16 transport: copy the reduced shard back as fp32)."""
        s, rem = self._split(a, b)
        work, fin = [], []
        if s > 0:
            main = flat[a:a + self.world * s]
            mine = flat[a + self.rank * s: a + (self.rank + 1) * s]
            # persistent transport buffers (one set per region: no allocation in the step); out of place is valid on
            # every backend
            if bf16:
                half = self._buf("rs.in", a, self.world * s, torch.bfloat16, flat.device)
                out = self._buf("rs.out", a, s, torch.bfloat16, flat.device)
                half.copy_(main)                                 # fp32 -> bf16 (round to nearest even)
                work.append(dist.reduce_scatter_tensor(out, half, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            else:
                out = self._buf("rs.out", a, s, flat.dtype, flat.device)
                work.append(dist.reduce_scatter_tensor(out, main, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            fin.append(lambda: mine.copy_(out))
        if rem < b:
            work.append(dist.all_reduce(flat[rem:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        return work, fin

    def _update_region(self, eng, a: int, b: int, lr, grad_scale, count, adam_kw, defer=None):
        """Adam on this rank's shard of region [a, b) (+ the replicated remainder), then the all-gather of the updated
        parameter shards (async; returned).  defer: a list - the all-gather is appended to it as a callable instead of
        being issued (collectives complete in issue order: optimizer_step issues the head's first when the decoder's
        may stay in flight under the next encoder forward)."""
        s, rem = self._split(a, b)
        work = []
        if s > 0:
            lo = a + self.rank * s
            eng.adam_step(lr, grad_scale, lo=lo, hi=lo + s, count=count, **adam_kw)
            count = False
            main = eng.ps.params[a:a + self.world * s]
            src = self._buf("ag.in", a, s, main.dtype, main.device)     # (in place all-gather is not valid on every backend)
            src.copy_(eng.ps.params[lo:lo + s])

            def gather():
                return dist.all_gather_into_tensor(main, src, group=self.group, async_op=True)
            if defer is None:
                work.append(gather())
            else:
                defer.append(gather)
        if rem < b:
            # the replicated remainder: every rank updates it, rank 0 alone adds it to the update / weight sums
            eng.adam_step(lr, grad_scale, lo=rem, hi=b, count=count,
                          **dict(adam_kw, track=bool(adam_kw.get("track")) and self.rank == 0))
        return work

    def finish(self, region=None):
        """Wait for the parameter all-gathers of the previous sharded step.  region = None: all of them (before anything
        reads the parameters); "head": only the encoder / bottleneck region - what the first forward plan reads; the
        decoder's shards may stay in flight under it until forward(before_decoder=self.finish) (TrainEngine.pack_dec_late)."""
        keep = []
        for tag, w in getattr(self, "_pending", []):
            if region is None or tag == region:
                self._wait(w, "params.all_gather" + ("" if tag == "head" else ".decoder"))
            else:
                keep.append((tag, w))
        self._pending = keep

    @staticmethod
    def _late(eng) -> bool:
        """May the decoder's parameter all-gather stay in flight under the first forward plan?  Only if that plan reads no
        decoder parameter: the engine packs the decoder's layouts at the head of fwd_b (pack_dec_late, no merged pack) and
        there IS a head region.  ONE predicate for optimizer_step (issue order) and forward (wait points).  Engine-level
        readers of the parameters between steps (eng.conditioning(), eng.encode(), tools) must call finish() first - the
        module surface does."""
        return eng.dec_grad_offset > 0 and bool(getattr(eng, "pack_dec_late", False)) and not getattr(eng, "merge_packs", False)

    def forward(self, eng, accum=None):
        """The forward of a sharded step: the encoder part starts as soon as ITS parameters are complete, the decoder's
        all-gather is waited for between the two forward plans.  accum: the micro-batch's fold in a group of accumulated
        ones (TrainEngine.forward): FIRST / ADD issue no statistics collective, LAST all-reduces the group's sums."""
        late = self._late(eng)
        self._warn_merged_packs(eng)
        self.finish("head" if late else None)
        kw = {} if accum is None else {"accum": accum}
        return eng.forward(self.allreduce_ema_async, before_decoder=self.finish if late else None, **kw)

    def backward_exchange(self, eng, bf16_grads: bool = False, accum_last: bool = False):
        """Backward with the sharded gradient exchange issued as the regions become final: decoder tail (reduce-scatter
        under the bottleneck / encoder backward), then the head.  optimizer_step() completes it.
        accum_last: this is the last micro-batch of a group of accumulated ones - every region takes the group's running
        sum in (TrainEngine.accum_grads, LAST, one launch over the region) in front of its reduce-scatter, so the
        exchange still overlaps the rest of the backward.  The earlier micro-batches of a group run the plain backward
        and exchange nothing."""
        n, lo = eng.ps.numel, eng.dec_grad_offset
        hi = getattr(eng, "dec_hi_offset", None)       # engines with two grouped wgrad launches: [hi, n) is final first
        flat = eng.ps.grads
        st = {"hi": hi}

        def reduce(a, b):
            if accum_last and b > a:
                eng.accum_grads(L.ACCUM_LAST, a, b)
            return self._reduce_region(flat, a, b, bf16_grads)

        def after_decoder_hi():
            self._guard_sync(eng)
            st["dec_hi"] = reduce(hi, n)

        def after_decoder():
            if "dec_hi" not in st:
                self._guard_sync(eng)
            st["dec"] = reduce(lo, n if "dec_hi" not in st else hi)

        self.allreduce_kl(eng)
        if hi is not None:
            eng.backward(after_decoder=after_decoder, after_decoder_hi=after_decoder_hi)
        else:
            eng.backward(after_decoder=after_decoder)
        if "dec" not in st:
            after_decoder()
        st["head"] = reduce(0, lo) if lo > 0 else ([], [])
        self._st = st

    def abandon_exchange(self):
        """Drop a sharded exchange no optimizer step will complete (an accumulated group discarded or started over
        unstepped): its collectives are waited for - they read the gradient buffer the next backward rewrites - and
        their results are not used."""
        st, self._st = self._st, None
        for key in ("dec_hi", "dec", "head"):
            for w in (st or {}).get(key, ([], []))[0]:
                w.wait()
        self._guard_wait()

    def _clip_norm_sharded(self, eng, regions, max_grad_norm: float, grad_scale: float, groups=None):
        """The clip coefficient of a sharded step, once every region is reduced: the sum of squares of this rank's shards
        (one launch), all-reduced over the ranks as ONE fp64 word, then a finalizing launch that adds the replicated
        remainders (the same values on every rank: counted once; empty ranges where a region has none).  Every rank sums
        the same words in the same order, so all hold the same coefficient bit for bit.
        groups (an Adam keyword: parameter groups): the norm covers the trainable tensors only - the shards and the
        remainders are cut to their element ranges (TrainEngine.trainable_ranges; more than 8: chained launches)."""
        shards, rems = [], []
        for a, b in regions:                             # the regions this step's backward_exchange reduced
            s, rem = self._split(a, b)
            shards.append((a + self.rank * s, a + (self.rank + 1) * s))
            rems.append((rem, b))
        if groups is not None:
            shards, rems = eng.trainable_ranges(groups, shards), eng.trainable_ranges(groups, rems)
        eng.grad_norm_step(shards, max_grad_norm, grad_scale, finalize=False)
        dist.all_reduce(eng.clip_sumsq[1:2], op=dist.ReduceOp.SUM, group=self.group)
        eng.grad_norm_step(rems, max_grad_norm, grad_scale, finalize=True, add_partial=True)

    def optimizer_step(self, eng, lr: float, grad_scale: float = 1.0, **adam_kw):
        """Sharded Adam + all-gather of the updated parameters (left in flight: finish() before the next forward).
        With max_grad_norm (an Adam keyword) the step first waits for ALL regions' reductions, computes the global norm
        (_clip_norm_sharded) and only then runs the shard / remainder Adam calls: the decoder's Adam no longer overlaps
        the head's reduction in such a step.  With track (an Adam keyword) the step ends with _ratios_sharded."""
        n, lo = eng.ps.numel, eng.dec_grad_offset
        st, self._st = self._st, None
        pend, counted, dec_end = [], True, n
        # late: the next forward waits for the head's parameters first and for the decoder's only between its two plans
        # (forward()); collectives complete in issue order, so the head's all-gather goes out first and the decoder's
        # right behind it.  Otherwise the decoder's all-gather is issued at once and runs under the head's Adam.
        late = self._late(eng)
        dec_gathers = [] if late else None
        self._guard_wait()
        clip = adam_kw.get("max_grad_norm")

        def reduced(key, what):
            """Wait for a region's reduction, then run its finishers; once per step (a second call finds nothing)."""
            work, fin = st[key]
            for w in work:
                self._wait(w, what)
            for f in fin:
                f()
            st[key] = ([], [])

        if clip is not None:
            for key, what in (("dec_hi", "grads.decoder_hi"), ("dec", "grads.decoder"), ("head", "grads.encoder")):
                if key in st:
                    reduced(key, what)
            regions = ([(st["hi"], n), (lo, st["hi"])] if "dec_hi" in st else [(lo, n)]) + [(0, lo)]
            self._clip_norm_sharded(eng, regions, clip, grad_scale, adam_kw.get("groups"))
            adam_kw = dict(adam_kw, norm_done=True)
        if "dec_hi" in st:                               # the upper layers' region: reduced under the rest of the chain
            reduced("dec_hi", "grads.decoder_hi")
            pend += [("dec", w) for w in self._update_region(eng, st["hi"], n, lr, grad_scale, True, adam_kw, dec_gathers)]
            counted, dec_end = False, st["hi"]
        reduced("dec", "grads.decoder")
        pend += [("dec", w) for w in self._update_region(eng, lo, dec_end, lr, grad_scale, counted, adam_kw, dec_gathers)]
        reduced("head", "grads.encoder")
        if lo > 0:
            pend += [("head", w) for w in self._update_region(eng, 0, lo, lr, grad_scale, False, adam_kw)]
        for g in dec_gathers or []:
            pend.append(("dec", g()))
        self._pending = pend
        if adam_kw.get("track"):
            self._ratios_sharded(eng)

    def _ratios_sharded(self, eng):
        """The update / weight ratios of a sharded step: this rank's chunk sums per tensor (one launch), all-reduced over
        the ranks as 2 P fp64 words, then the finalizing launch that reads those words alone.  Every rank receives the
        same words, so all hold the same ratios bit for bit - without waiting for the parameter all-gathers."""
        eng.ratio_step(finalize=False)
        dist.all_reduce(eng.uw_sums[:2 * eng.uw_n], op=dist.ReduceOp.SUM, group=self.group)
        eng.ratio_step(finalize=True, add_partial=True)

    def train_step_sharded(self, eng, lr: float, grad_scale: float = 1.0, bf16_grads: bool = False, **adam_kw):
        """forward + backward + sharded optimizer step (see the module docstring).  Every rank ends with the same
        parameters as train_step() gives (fp32 transport: up to summation order; bf16 transport: the summed gradient
        is rounded to bf16 once per hop).  The Adam MOMENTS of a rank are valid for its own shards only (ZeRO-1): use
        gather_moments() before reading them (checkpoints)."""
        if self._solo():
            eng.forward()
            eng.backward()
            eng.adam_step(lr, grad_scale, **adam_kw)
            return
        self.forward(eng)
        self.backward_exchange(eng, bf16_grads)
        self.optimizer_step(eng, lr, grad_scale, **adam_kw)

    @staticmethod
    def _regions(eng):
        """The regions of the flat buffer the sharded schedule exchanges separately (each has its own shard layout):
        [upper decoder layers + post network |] decoder | encoder + bottleneck."""
        n, lo, hi = eng.ps.numel, eng.dec_grad_offset, getattr(eng, "dec_hi_offset", None)
        return [(hi, n), (lo, hi), (0, lo)] if hi is not None else [(lo, n), (0, lo)]

    def gather_moments(self, eng):
        """All-gather the Adam moments (each rank holds valid moments for its own shards only under the sharded step) and,
        where the optimizer keeps them, the averaged weights, which follow the same rule.  COLLECTIVE: every rank must
        call it."""
        if self._solo():
            return
        for a, b in self._regions(eng):
            s, rem = self._split(a, b)
            if s > 0:
                for buf in eng.opt_buffers():
                    dist.all_gather_into_tensor(buf[a:a + self.world * s], buf[a + self.rank * s: a + (self.rank + 1) * s].clone(),
                                                group=self.group)
        self.moments_complete_at(eng.step_count)

    def moments_complete_at(self, step: int):
        """Every rank holds ALL Adam moments (and the whole average) of this engine step: after a gather, after an
        all-reduce step, after every rank restored the same complete state (FusedAdam.load_state_dict)."""
        self.moments_step = int(step)

    def moments_complete(self, eng) -> bool:
        """Does this rank hold the Adam moments of ALL parameters for the engine's current step?  (Always under the
        all-reduce schedule; under the sharded one only right after gather_moments().)"""
        return self._solo() or not self.sharded or eng.step_count == 0 or self.moments_step == eng.step_count

    def sync_optimizer_state(self, model):
        """Make model / optimizer state readable on every rank: waits for the parameter all-gathers in flight and
        all-gathers the sharded Adam moments.  COLLECTIVE - call it on ALL ranks before any of them calls
        optimizer.state_dict() / checkpoint.save() (checkpoint.save does it when the model is attached)."""
        self.finish()
        eng = getattr(model, "_engine", None)
        if eng is not None and self.sharded and not self._solo() and not self.moments_complete(eng):
            self.gather_moments(eng)

    def allreduce_ema_async(self, z_sum: torch.Tensor, n_sum: torch.Tensor):
        """Like allreduce_ema but returns the work handle (the engine then defers the EMA accumulation)."""
        if self._solo():
            return None
        both = self._ema_flat(z_sum, n_sum)
        if both is None:
            self.allreduce_ema(z_sum, n_sum)
            return None
        return dist.all_reduce(both, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    @staticmethod
    def _ema_flat(z_sum, n_sum):
        if z_sum.is_contiguous() and n_sum.is_contiguous() and \
                n_sum.data_ptr() == z_sum.data_ptr() + z_sum.numel() * z_sum.element_size() and \
                z_sum.untyped_storage().data_ptr() == n_sum.untyped_storage().data_ptr():
            return torch.as_strided(z_sum, (z_sum.numel() + n_sum.numel(),), (1,))
        return None

    def allreduce_ema(self, z_sum: torch.Tensor, n_sum: torch.Tensor):
        if self._solo():
            return
        # the engine allocates n_sum right behind z_sum: one collective instead of two
        both = self._ema_flat(z_sum, n_sum)
        if both is not None:
            dist.all_reduce(both, op=dist.ReduceOp.SUM, group=self.group)
            return
        dist.all_reduce(z_sum, op=dist.ReduceOp.SUM, group=self.group)
        dist.all_reduce(n_sum, op=dist.ReduceOp.SUM, group=self.group)

    def broadcast_codebook(self, eng, src: int = 0):
        """The EMA codebook state (emb, ema_numer, ema_denom) of rank `src` to every rank.  COLLECTIVE."""
        if eng.bn_type == "vqvae-ema":
            for t in (eng.emb, eng.ema_numer, eng.ema_denom):
                dist.broadcast(t, src, group=self.group)

    def broadcast_params(self, eng, src: int = 0):
        self.finish()
        dist.broadcast(eng.ps.params, src, group=self.group)
        self.broadcast_codebook(eng, src)

    def restart_codes(self, eng, min_usage: float, call: int, src: int = 0, **kw):
        """TrainEngine.restart_codes under data parallel.  COLLECTIVE: every rank runs the launch (the same plans on every
        rank; ema_denom is replicated, so the dead list and the counts are the same everywhere) - only the rows differ,
        each rank seeding from its own batch - and rank `src`'s codebook state is then broadcast: the replicas end up bit
        equal to a single process that saw that rank's batch.  The counts and the (code, row) pairs travel with it: each
        rank's launch is gated by its own chain_guard word, whose cross-rank maximum may still be in flight here, so on a
        guarded step the ranks' own counts could differ - after the broadcast restart_out() / restart_pairs() describe, on
        every rank, the codebook every rank holds.  The broadcasts are blocking collectives issued behind the launch on the
        compute stream, like broadcast_params; they happen on restart steps only."""
        eng.restart_codes(min_usage, call, **kw)
        if not self._solo():
            self.broadcast_codebook(eng, src)
            for t in (eng.restart_out(), eng.restart_pairs()):
                dist.broadcast(t, src, group=self.group)

    def sum_eval_record(self, acc: torch.Tensor, hist: torch.Tensor):
        """The ranks' evaluation records (aew_eval_acc_t: acc float64 [16], hist uint32 counts held as int32 [K]) summed
        in ONE all-reduce.  COLLECTIVE.  The counts are widened to int64 (the int32 tensor holds unsigned words) and
        travel in the float64 buffer of the sums, where integers under 2^53 - and so their sum - are exact.  Returns
        (acc float64 [16], hist int64 [K]); the arguments are left alone."""
        n = acc.numel()
        buf = self._buf("eval", 0, n + hist.numel(), torch.float64, acc.device)
        buf[:n].copy_(acc)
        buf[n:].copy_(hist.to(torch.int64) & 0xffffffff)
        if not self._solo():
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        return buf[:n].clone(), buf[n:].to(torch.int64)

    def eval_finish(self, eng) -> torch.Tensor:
        """TrainEngine.eval_finish over the sum of every rank's record.  COLLECTIVE: the summed record takes the place of
        this rank's own for the finalize launch and the rank's own is put back behind it (all on the compute stream), so
        evaluation may go on and a second call does not count anything twice.  Counts saturate at 2^32 - 1."""
        eng.eval_plans()
        own = eng.eval_acc.clone(), eng.eval_hist.clone()
        acc, hist = self.sum_eval_record(*own)
        hist = hist.clamp_(max=0xffffffff)
        eng.eval_acc.copy_(acc)
        eng.eval_hist.copy_(torch.where(hist >= 2 ** 31, hist - 2 ** 32, hist))       # back to unsigned words in int32
        out = eng.eval_finish().clone()
        eng.eval_acc.copy_(own[0])
        eng.eval_hist.copy_(own[1])
        return out

    def sum_eval_group_record(self, gacc: torch.Tensor, gtot: torch.Tensor, ghist: Optional[torch.Tensor]):
        """The ranks' grouped evaluation records (aew_eval_groups_t: gacc float64 [G][8], gtot float64 [4], ghist uint32
        counts held as int32 [G][K], or None without a codebook) summed in ONE all-reduce.  COLLECTIVE.  Like
        sum_eval_record: the counts are widened to int64 and travel in the float64 buffer of the sums, where integers
        under 2^53 are exact.  Returns (gacc, gtot, ghist int64 or None); the arguments are left alone."""
        na, nt = gacc.numel(), gtot.numel()
        nh = ghist.numel() if ghist is not None else 0
        buf = self._buf("eval_groups", 0, na + nt + nh, torch.float64, gacc.device)
        buf[:na].copy_(gacc.reshape(-1))
        buf[na:na + nt].copy_(gtot)
        if nh:
            buf[na + nt:].copy_(ghist.reshape(-1).to(torch.int64) & 0xffffffff)
        if not self._solo():
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        return (buf[:na].clone().view_as(gacc), buf[na:na + nt].clone(),
                buf[na + nt:].to(torch.int64).view_as(ghist) if nh else None)

    def eval_group_finish(self, eng):
        """TrainEngine.eval_group_finish over the sum of every rank's grouped record.  COLLECTIVE: like eval_finish, the
        summed record takes the place of this rank's own for the finalize launch and the rank's own is put back behind
        it.  Counts saturate at 2^32 - 1.  Returns copies of (gout, tout)."""
        own = eng.eval_gacc.clone(), eng.eval_gtot.clone(), (eng.eval_ghist.clone() if eng.eval_ghist is not None else None)
        gacc, gtot, ghist = self.sum_eval_group_record(*own)
        eng.eval_gacc.copy_(gacc)
        eng.eval_gtot.copy_(gtot)
        if ghist is not None:
            ghist = ghist.clamp_(max=0xffffffff)
            eng.eval_ghist.copy_(torch.where(ghist >= 2 ** 31, ghist - 2 ** 32, ghist))      # back to unsigned words in int32
        gout, tout = eng.eval_group_finish()
        out = gout.clone(), tout.clone()
        eng.eval_gacc.copy_(own[0])
        eng.eval_gtot.copy_(own[1])
        if ghist is not None:
            eng.eval_ghist.copy_(own[2])
        return out

    def attach(self, model, sharded: bool = False, bf16_grads: bool = False):
        """Hook the collectives into the module surface.  sharded=False: loss.backward() leaves the fully reduced
        gradients in every .grad (any optimizer).  sharded=True: backward issues the reduce-scatter, FusedAdam.step()
        updates this rank's shards and all-gathers the parameters (model.run waits for them); .grad then holds the
        reduced values for this rank's shards only, so only FusedAdam may be used."""
        model._dp = self
        self.sharded, self.bf16_grads = bool(sharded), bool(bf16_grads)
        model._ema_allreduce = self.allreduce_ema_async if sharded else self.allreduce_ema
        if getattr(model, "_engine", None) is not None:
            self.prepare_vae(model._engine)
