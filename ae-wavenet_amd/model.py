"""Training-step engine behind the drop-in module surfaces.

`TrainEngine` owns the workspace, the flat parameter / gradient buffers and the forward /
backward / optimizer plans for one (model, batch size, window).  `autoencoder_model.AutoEncoder`
and `mfcc_inverter.MfccInverter` wrap it in the reference's nn.Module surface
(autoencoder_model.py:206-259, mfcc_inverter.py:89-108); `bench.py` drives it directly.
"""
from __future__ import annotations

import ctypes as C
import os

import math
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from .engine import (F3, BottleneckPlan, DecoderPlan, EncoderPlan, Packer, ParamStore, TAG_ADAM, TAG_LOSS, TAG_PACK, TAG_UPS, TAG_VQ,
                     bottleneck_param_specs, decoder_param_specs, encoder_param_specs, reduce_op)
from .plan import CopyTableBuilder, Mat, Plan, Workspace, insert_nt_chains, pinned_upload, ru, split_small_nt

MEAN_LOSS = {"none": True, "ae": True, "vae": True, "vqvae": False, "vqvae-ema": False}


_SERIAL = [0]


class OptState(NamedTuple):
    """The optimizer state of a model away from an engine: what TrainEngine.opt_state() hands out and load_opt_state()
    takes in, what the module surface carries between engines and what FusedAdam reads / restores checkpoints through."""
    step: int                             # optimizer steps taken
    m: torch.Tensor                       # first / second moments, flat fp32 [ps.numel]
    v: torch.Tensor
    avg_steps: int = 0                    # averaged steps taken
    avg: Optional[torch.Tensor] = None    # averaged weights, flat like m / v; None = no average
    averaged_in: bool = False             # the average sits in the parameters' place, `avg` holds the raw ones
    complete: bool = True                 # False: taken from a sharded data-parallel engine without a gather - valid for
                                          # that rank's shards only

    def to(self, device) -> "OptState":
        return self._replace(m=self.m.to(device), v=self.v.to(device), avg=None if self.avg is None else self.avg.to(device))


class TrainEngine:
    """kind: 'autoencoder' | 'mfcc_inverter'.

    loss_mode (vqvae-ema only): 'intended' = rec.sum() + com.sum() (vqema_bn.py:244);
    'head' = commitment only, the debug state HEAD ships (vqema_bn.py:246, SURVEY C-3).
    take_compat: reproduce the reference's torch.take jitter gather (SURVEY C-1).
    update_codebook_every_step: refresh emb from the EMA statistics each step (standard
    VQ-VAE-EMA); the reference only refreshes at global_step == 10000 (chassis.py:175-176).
    """
    DIAG_LANE = 3             # codebook diagnostics (behind vq.ema on the same lane; read at the end of the forward)
    LANE_PACK_DEC = 1         # side lane of the decoder's forward-layout weight pack (joined by the end of fwd_a) ...
    pack_dec_late = True      # the decoder's weight pack at the head of fwd_b instead of fwd_a (see _place_decoder_pack: data-parallel overlap)
    small_split = 0           # > 0: bf16 NT launches of few 64 x 64 blocks contract K as up to 8 ranges on separate workgroups, as
                              # long as ranges x blocks stays at or under this (aew_gemm_nt_t.k_split hint, plan.split_small_nt)
    merge_packs = None        # True: all weight-layout packs of a step as ONE copy-table launch at the head of fwd_a (three launches
                              # fewer: 6.837 -> 6.802 ms per step interleaved, r05).  None = on unless the process is a rank of a
                              # data-parallel group: there the decoder's pack stays at the head of fwd_b (pack_dec_late), so that
                              # the decoder's parameter all-gather can run under the encoder forward (dp.DataParallel.forward)
    graph_lanes = 2           # lane mode of graph captures when the process-wide mode is 0 (aew_set_lanes): 2 = lanes 4 / 5 are
                              # branches, everything else in plan order.  Eager runs stay serial (one cross-stream edge costs
                              # more there than the branch returns: 7.27 vs 6.90 ms per step).  0: never
    LANE_PACK_LATE = 2        # ... and of the backward-layout pack at the head of fwd_b (joined by its end).  4 / 5: the lanes
                              # aew_set_lanes(2) honours alone (A/B: each a single fork / join, profiles/r04_notes.md §16)
    PACK_LANE = 2             # side lane of the forward-layout weight pack (layers 1.. of the encoder, biases, bottleneck)
    nt_chain = 64             # chained NT launches (AEW_OP_NT_CHAIN, csrc/aew_chain.hip): runs of dependent NT ops of the decoder
                              # FORWARD - the gated stack's G1 / G2 ops (wavenet.py:354-357), the post network's pair - as
                              # launches of up to this many stages with tile-granular hand-off (64: the whole stack is ONE
                              # launch of 27 856 tiles instead of 39; 2: the pair of a layer; 0: one launch per op).  Bit-identical
                              # results; per-op timing (aew_timing_enable(1)) always runs the ops one by one.  Measured,
                              # interleaved on one box: fwd_b plan 2.089 -> 1.911 ms, step 6.865 -> 6.748 ms (profiles/r05_notes.md)
    nt_chain_bwd = (64, (128, 256))   # the same for the BACKWARD's d.post / dz / dx run: (stages per launch, rows per tile), rows = 256,
                              # 128, or (rows of d.post / dz, rows of dx); a plain number means 256-row tiles; 0: one launch per op.
                              # On 256-row tiles a dz stage is 320-448 tiles - fewer than the 512 resident slots - so its consumers
                              # (dx) are resident before it has finished and 10 000 of the launch's 21 072 tiles spin on a counter.
                              # dz on 128-row tiles (aew_nt_chain_build_bm; same bits) is 640-896 tiles per stage, the forward's
                              # range: 612 tiles wait.  dx stays on 256 rows: its K loop is 4 x the dz width, and a half-height
                              # tile stages W once more per 256 rows - 128 rows throughout leaves 7 tiles waiting and is slower.
                              # Measured, interleaved on one box (profiles/chain_bm.txt): bwd plan 4.27 stand-alone, 3.99 chained
                              # on 256, 4.08 on 128, 3.93 ms dz 128 / dx 256; step 6.56 / 6.37 / 6.53 / 6.35 ms.  A rank of a
                              # data-parallel group keeps the backward unchained (_chain_args)
    nt_chain_bwd_phase = 0    # with nt_chain_bwd = 2: 0 pairs (dz.l, dx.l); 1 pairs (dx.l, dz.l-1) - the dependency whose producer stage is
                              # larger than the 512 resident tiles, so that its consumers find it finished
    nt_chain_max_stage_tiles = 2048   # runs whose stages average more tiles than this (four waves of the 512 resident slots) stay
                              # stand-alone launches: the deep decoder (30 x 512, 64k windows: 8 224 tiles per gated stage) loses
                              # 1 % to chaining (62.9 vs 62.2 ms per step) - nothing to gain at 16 tile waves per launch, and the
                              # hand-off (write-through stores, one acquire per tile) is not free.  0 = no limit
    nt_chain_force = False    # tests: chain also the sizes the stand-alone launcher runs on its small-launch shapes
    nt_chain_flags = 0        # aew_nt_chain_t.flags (measurement aids)
    nt_chain_spin_max = 0     # polls before a hand-off wait gives up (0: the library's 1 << 18, ~0.3 s)
    diag_early = True         # per-step diagnostics placed where their inputs become final (False: at the tail of the
                              # forward plan; A/B: 8.02 -> 7.99 ms per step)

    def __init__(self, hps, B: int, device, n_mel: Optional[int] = None, loss_mode: str = "intended",
                 take_compat: bool = False, update_codebook_every_step: bool = True, impl: int = 0,
                 n_win: Optional[int] = None, use_graphs: Optional[bool] = None, wgrad_group: Optional[int] = None,
                 tuning=None):
        self.hps, self.B, self.impl = hps, B, impl
        _SERIAL[0] += 1
        self.serial = _SERIAL[0]          # unique per engine (id() can be recycled after garbage collection)
        self.weights_version = 0          # bumped by adam_step(): FusedAdam writes parameters by raw pointer
        # plans run as captured hipGraphs unless told otherwise.  An explicit constructor argument wins; the environment
        # (AEW_USE_GRAPHS=0: eager stream launches, AEW_WGRAD_GROUP=n: layers per grouped wgrad launch, 0 = round 2's one
        # op per matrix) only supplies the default of an argument left at None (A/B and bisecting aid).
        if use_graphs is None:
            use_graphs = os.environ.get("AEW_USE_GRAPHS", "1") == "1"
        self.use_graphs = bool(use_graphs)
        if wgrad_group is None:
            wgrad_group = int(os.environ["AEW_WGRAD_GROUP"]) if os.environ.get("AEW_WGRAD_GROUP") is not None \
                else DecoderPlan.wgrad_group
        self.wgrad_group = int(wgrad_group)
        self.tuning = tuning              # _lib.Tuning (aew_tuning_t) for this engine's launches, or None
        self.merge_packs_auto = self.merge_packs is None          # (dp.DataParallel warns when an automatic choice went the
        if self.merge_packs is None:                              #  wrong way: engine built before init_process_group)
            import torch.distributed as _dist
            self.merge_packs = not (_dist.is_available() and _dist.is_initialized() and _dist.get_world_size() > 1)
        self.kind = hps.global_model
        self.bn_type = hps.bn_type if self.kind == "autoencoder" else "none"
        self.loss_mode, self.take_compat = loss_mode, take_compat
        self.update_codebook_every_step = update_codebook_every_step
        self.device = torch.device(device)
        self.n_win = n_win or hps.n_win_batch
        with_enc = self.kind == "autoencoder"
        self.geom = G.model_geometry(hps, with_enc, self.n_win)
        self.n_mel = n_mel if n_mel is not None else hps.n_lc_in if not with_enc else 3 * hps.n_mfcc
        self.ws = ws = Workspace(self.device)
        g = self.geom
        # ---- parameters
        dec_pre = "decoder." if with_enc else "wavenet."
        specs = []
        if with_enc:
            specs += encoder_param_specs(self.n_mel, hps.enc_n_out)
            specs += bottleneck_param_specs(hps)
        specs += decoder_param_specs(hps, hps.n_lc_in, dec_pre)
        self.ps = ps = ParamStore(ws, specs)
        self.dec_pre = dec_pre
        # ---- static inputs
        self.in_wav = ws.alloc("in.wav", B * g.enc_in_len, torch.float32)[:B * g.enc_in_len].view(B, g.enc_in_len)
        self.in_mel = ws.alloc("in.mel", B * self.n_mel * g.mel_len, torch.float32)[:B * self.n_mel * g.mel_len] \
            .view(B, self.n_mel, g.mel_len)
        self.in_voice = ws.alloc("in.voice", B, torch.int64)[:B]
        self.in_jitter = ws.alloc("in.jitter", B * g.embed_len, torch.int64)[:B * g.embed_len].view(B, g.embed_len)
        self.loss_buf = ws.alloc("loss", 8, torch.float32)
        # upstream gradient d(L)/d(loss) of the current backward call (autograd's `g`): the ops where the loss
        # gradient enters the backward read it from device memory, so (loss * k).backward() scales every gradient
        # without a host sync and without touching the captured graphs
        self.gmul = ws.alloc("loss.gmul", 4, torch.float32)
        self.gmul[:1].fill_(1.0)
        # STICKY word of the chained launches (aew_nt_chain_t.sticky): no plan clears it; a hand-off wait that gave up leaves
        # (stage + 1) here, and the optimizer / EMA ops read it as their guard - the step does not reach the parameters
        self.chain_guard = ws.alloc("chain.guard", 4, torch.int32)
        # ---- tables
        # encoder / bottleneck tables stay on the main lane (their packed weights are needed at once and
        # their gradients come last); the decoder's are side-lane work: its weight pack overlaps the
        # (tiny-grid) encoder forward, its gradient unpack overlaps the encoder backward
        self.pack_tbl = CopyTableBuilder(ws, "tbl.pack")
        self.unpack_tbl = CopyTableBuilder(ws, "tbl.unpack")
        self.pack_dec = CopyTableBuilder(ws, "tbl.pack_dec")
        self.unpack_dec = CopyTableBuilder(ws, "tbl.unpack_dec")
        self.in_tbl = CopyTableBuilder(ws, "tbl.in")
        self.pack_late = CopyTableBuilder(ws, "tbl.pack_late")      # dgrad layouts of the encoder weights: backward only
        # the encoder's first layer waits for its own (small) weight pack only; the rest of the forward-layout packs
        # (57 MB of fp32 encoder weights, biases, bottleneck) run on a side lane under layer 0
        self.pack_first = CopyTableBuilder(ws, "tbl.pack_first") if with_enc else None
        self.pk = Packer(ps, self.pack_tbl, self.unpack_tbl, late_tbl=self.pack_late, first_tbl=self.pack_first)
        self.pk_dec = Packer(ps, self.pack_dec, self.unpack_dec)
        Mp = ru(self.n_mel, 64)
        self.mel_cl = Mat.new(ws, "mel_cl", B, g.mel_len, Mp, F3)
        self.in_tbl.add(self.in_mel.data_ptr(), self.mel_cl.ptr, [B, g.mel_len, self.n_mel],
                        [self.n_mel * g.mel_len, 1, g.mel_len], [self.mel_cl.bs, Mp, 1], F3, F3)
        # ---- sub-plans
        self.enc: Optional[EncoderPlan] = None
        self.bn: Optional[BottleneckPlan] = None                   # (the mfcc inverter has neither)
        if with_enc:
            self.enc = EncoderPlan(ws, ps, hps, g, B, self.n_mel, self.mel_cl, self.pk, impl, in_tbl=self.in_tbl,
                                   in_mel=self.in_mel, wgrad_group=self.wgrad_group)
            self.bn = BottleneckPlan.make(self.bn_type, ws, ps, hps, g, B, self.enc, self.pk, impl, loss_mode)
        self.dec = DecoderPlan(ws, ps, hps, g, B, dec_pre, hps.n_lc_in, self.bn.code if with_enc else self.mel_cl, self.in_wav,
                               self.in_voice, self.in_jitter, take_compat, self.pk_dec, impl, wgrad_group=self.wgrad_group)
        self._build()
        # the bottleneck's buffers (and the codebook plan `cb`) under the names the module surface, the data-parallel
        # wrapper, bench.py and the tests read: plain attributes, present exactly where the type has them
        for name in self.bn.names if self.bn is not None else ():
            setattr(self, name, getattr(self.bn, name))
        self.adam_state = None
        self.step_count = 0

    # --------------------------------------------------------------------------------------
    # plan construction: _build runs the stages below in the order of the workspace allocations they make (device
    # addresses; pinned with every op they emit by tests/data/plan_parent.json)
    # --------------------------------------------------------------------------------------
    def _build(self):
        B, w = self.B, self.n_win
        self.fwd_a, self.fwd_b, self.bwd = Plan("fwd_a"), Plan("fwd_b"), Plan("bwd")
        nll = (self.dec.nll.data_ptr(), B * w, 1.0 / (B * (w - 1)) if MEAN_LOSS[self.bn_type] else 1.0)   # the loss's NLL term
        chain_kw = self._chain_args()
        self._build_forward_a()
        self._build_forward_b(nll, chain_kw)
        self._build_backward(nll[2], chain_kw)
        self._split_small()
        dec_packed = self._place_decoder_pack()
        self._cut_plans()
        if self.bn is not None:
            self.bn.build_codebook()
        self._place_packs(dec_packed)
        self._build_optimizer()
        self._declare_lazy()

    def _chain_args(self) -> dict:
        """Stages per chained launch of the forward / backward as applied (nt_chain_used / nt_chain_bwd_used) and the
        keywords every insert_nt_chains call of this engine shares."""
        # AEW_NT_CHAIN = "f", "f,b" or "f,b,bm": stages per chained launch of the forward / backward and the backward's
        # row-tile height, 256 where it is left out (A/B and bisecting aid)
        env = os.environ.get("AEW_NT_CHAIN")
        n_b, bm_b = self.nt_chain_bwd if isinstance(self.nt_chain_bwd, (tuple, list)) else (self.nt_chain_bwd, 256)
        n_f, n_b = int(self.nt_chain), int(n_b)
        if env is not None and env.strip():
            try:
                v = [int(x) for x in env.split(",") if x.strip()]
            except ValueError:
                raise ValueError(f"AEW_NT_CHAIN={env!r}: expected 'f', 'f,b' or 'f,b,bm' (stages per chained launch, forward / "
                                 "backward; rows per tile of the backward's)")
            if v:
                n_f, n_b, bm_b = v[0], (v[1] if len(v) > 1 else 0), (v[2] if len(v) > 2 else 256)
        # a rank of a data-parallel group keeps the backward unchained: the cross-rank maximum of the guard word is issued
        # before the second half of the decoder backward runs (dp.DataParallel._guard_sync), so a hand-off that gave up there
        # would stop the update on its own rank only
        if n_b and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            n_b = 0
        bm_dz, bm_dx = (bm_b if isinstance(bm_b, (tuple, list)) else (bm_b, bm_b))
        if int(bm_dz) not in (128, 256) or int(bm_dx) not in (128, 256):
            raise ValueError(f"rows per tile of the backward chain = {bm_b!r}: 256, 128 or a pair of them")
        self.nt_chain_bwd_bm_used = (int(bm_dz), int(bm_dx))
        self.nt_chain_used = n_f if self.impl == 0 else 0
        self.nt_chain_bwd_used = n_b if self.impl == 0 else 0
        return dict(force=bool(self.nt_chain_force), flags=int(self.nt_chain_flags), max_stage_tiles=int(self.nt_chain_max_stage_tiles),
                    sticky_ptr=self.chain_guard.data_ptr(), tuning=self.tuning, spin_max=int(self.nt_chain_spin_max))

    def _build_forward_a(self):
        """fwd_a: inputs, encoder, bottleneck up to the EMA statistics (the weight packs go in front: _place_packs)."""
        fa = self.fwd_a
        self.in_tbl.emit(fa, "mel->channels-last")
        if self.enc is not None:
            self.enc.build_forward(fa, join_before_layer1=("lane", self.PACK_LANE) if self.pack_first is not None else False)
            self.bn.build_forward(fa, self.fwd_b)

    def _build_diagnostics(self):
        """Per-step diagnostics (what the reference's loss modules report, vqema_bn.py:251-264, chassis.py:266-270): side-lane
        ops placed where their inputs become final, not after the plan's last op (a side op starts after every main-lane
        op that precedes it in the plan: appended at the end they were ~0.09 ms of exposed tail):
          codebook / encoder-output statistics  right here, under the whole decoder forward
          peak log-probability statistics       after the logits GEMM, under the softmax
          rec / tprb_m / com                    after the softmax, under the loss reduction
        Returns the two hooks (after_logits, after_nll) that place the latter two."""
        ws, hps, B, w, fb = self.ws, self.hps, self.B, self.n_win, self.fwd_b
        n_pos_m = B * (w - 1)
        self.diag = ws.alloc("diag.out", 16, torch.float32)              # [0..5] (vqema_bn.py:254-260)
        self.diag_pk = ws.alloc("diag.peak", 16, torch.float32)          # [6..8] (vqema_bn.py:261-263)
        self.diag_scratch = ws.alloc("scratch.diag", 512, torch.float32)
        self.diag_scratch_pk = ws.alloc("scratch.diag_pk", 512, torch.float32)   # (the two diagnostics ops may overlap on lanes)
        self.met_buf = ws.alloc("diag.metrics", 8, torch.float32)        # [1] rec, [2] tprb_m, [3] com
        if self.bn is not None:
            self.bn.build_diag(fb, self.DIAG_LANE, w, self.diag_scratch, self.diag)   # not lane 1: decoder layer 0 waits for that one
        # peak statistics of the predicted distribution (vqema_bn.py:261-263).  With the reference's 256 classes the
        # softmax kernel has each row in registers and writes the per-position peak log-probability / arg-max next to the
        # nll; the diagnostics op then reduces 2 x 160 KB instead of reading the 41 MB of logits a second time
        fused_peak = hps.n_quant == 256 and self.dec.Qp == 256
        if fused_peak:
            self.peak_buf = ws.alloc("diag.peak_pos", B * w, torch.float32)
            self.amax_buf = ws.alloc("diag.amax_pos", B * w, torch.int32)
            self.dec.peak_ptrs = (self.peak_buf.data_ptr(), self.amax_buf.data_ptr())

        def peak_diag(plan):
            dg = L.VqDiag()
            lgm = self.dec.logits
            dg.logits, dg.bs, dg.pitch, dg.B, dg.w, dg.n_quant = lgm.ptr, lgm.bs, lgm.pitch, B, w, hps.n_quant
            dg.scratch, dg.out = self.diag_scratch_pk.data_ptr(), self.diag_pk.data_ptr()
            if fused_peak:
                dg.peak, dg.amax = self.dec.peak_ptrs
            with plan.side(1):
                plan.add(L.OP_VQ_DIAG, dg, "diagnostics (peak)", TAG_LOSS)

        def after_logits(plan):
            if not fused_peak:
                peak_diag(plan)

        def after_nll(plan):
            if fused_peak:
                peak_diag(plan)
            mterms = [(self.dec.nll.data_ptr(), B * w, 1.0 / n_pos_m), (self.dec.ptgt.data_ptr(), B * w, 1.0 / n_pos_m)]
            if self.bn is not None:
                mterms += self.bn.metric_terms()
            with plan.side(1):
                plan.add(L.OP_REDUCE, reduce_op(mterms, self.met_buf.data_ptr()), "metrics", TAG_LOSS)
        return after_logits, after_nll

    def _build_forward_b(self, nll, chain_kw: dict):
        """fwd_b (behind the bottleneck's vq.ema): backward-layout weight pack, diagnostics, decoder, chained launches, loss."""
        fb = self.fwd_b
        if not self.merge_packs:
            late = Plan("pack_late")
            with late.side(self.LANE_PACK_LATE):               # only the backward reads these: hidden under the decoder
                self.pack_late.emit(late, "pack weights (backward layouts)")
            fb.splice(len(fb.ops), late, TAG_PACK)
        hooks = self._build_diagnostics()
        if self.diag_early:
            self.dec.build_forward(fb, after_logits=hooks[0], after_nll=hooks[1])
        else:                                                  # A/B: all of them after the plan's last main-lane op
            self.dec.build_forward(fb)
        if self.nt_chain_used >= 2:
            insert_nt_chains(fb, self.ws, "chain.fwd", lambda lab: lab.startswith(("G1.", "G2.", "post1", "post2")),
                             max_len=self.nt_chain_used, **chain_kw)
        red = self.bn.loss_op(nll) if self.bn is not None else reduce_op([nll], self.loss_buf.data_ptr())
        fb.add(L.OP_REDUCE, red, "loss", TAG_LOSS)
        for hook in () if self.diag_early else hooks:
            hook(fb)

    def _build_backward(self, scale: float, chain_kw: dict):
        """bwd: decoder, bottleneck, encoder, the gradient unpacks and statistics.  scale: the loss's mean / sum factor."""
        ws, hps, B, bw = self.ws, self.hps, self.B, self.bwd
        bw.zero(ws, "grads")
        nll_scale = self.bn.nll_scale(scale) if self.bn is not None else scale
        self.dec.build_backward(bw, nll_scale, early_tbl=CopyTableBuilder(ws, "tbl.unpack_dec_early"))
        if self.nt_chain_bwd_used >= 2:
            heads = ("d.post2", "d.post1")[int(self.nt_chain_bwd_phase):]    # (phase 1: pairs are (dx.l, dz.l-1), not (dz.l, dx.l))
            insert_nt_chains(bw, ws, "chain.bwd", lambda lab: lab.startswith(heads + ("dz.", "dx.")),
                             max_len=self.nt_chain_bwd_used, **chain_kw,
                             bm=lambda lab: self.nt_chain_bwd_bm_used[1 if lab.startswith("dx.") else 0])
        # gradient statistics of run() (autoencoder_model.py:252-257 mel_grad_sd / bn_grad_sd; mfcc_inverter.py:100-106
        # mel_grad_sd / mel_grad_mean): by-products of this backward, reduced on a side lane as soon as their input is
        # final (d(loss)/d(code) here, under the encoder backward)
        self.gstat = ws.alloc("diag.gstat", 8, torch.float32)            # [0:4] mel (mean, std, sum, sumsq), [4:8] bn

        def moments(mat, cols, slot, nm):
            mo = L.Moments()
            mo.x, mo.rows, mo.cols, mo.batch = mat.view(), mat.rows, cols, B
            mo.out = self.gstat.data_ptr() + 4 * slot
            with bw.side(1):
                bw.add(L.OP_MOMENTS, mo, f"grad stats ({nm})", TAG_LOSS)
        with bw.side(self.dec.tail_lane_used or 1):                 # after every decoder wgrad on any side lane
            self.unpack_dec.emit(bw, "unpack grads (decoder)", join=True)
        if self.enc is not None:
            dcode = self.dec.dlc_src                      # d(loss)/d(code) [B][Ne][dp]
            moments(dcode, hps.bn_n_out, 4, "bn")
            self.bn.build_backward(bw, dcode)
            self.enc.build_backward(bw, need_input_grad=True)
        # (mel gradient statistics: its input is the last thing the backward writes)
        moments(self.enc.dy[0] if self.enc is not None else self.dec.dlc_src, self.n_mel, 0, "mel")
        self.unpack_tbl.emit(bw, "unpack grads", join=True)        # reads the side-lane encoder wgrad slabs

    def _split_small(self):
        """Launches of a few dozen 64 x 64 blocks (the upsampler / encoder data gradients): split-K hint."""
        self.small_split_made = []
        if int(self.small_split) > 0 and self.impl == 0:
            for pl in (self.fwd_a, self.fwd_b, self.bwd):
                self.small_split_made += split_small_nt(pl, self.ws, "ks." + pl.name, int(self.small_split))

    def _place_decoder_pack(self) -> bool:
        """The decoder's weight layouts are packed at the head of fwd_b (behind vq.ema), not of fwd_a: nothing in fwd_a
        reads a decoder parameter, so a data-parallel caller lets the all-gather of the updated decoder shards run
        under the encoder forward and waits for it only between the two plans (forward(before_decoder=...)).  Serial
        plans: the same launches in the same total time.  Returns whether the pack was placed here."""
        fb = self.fwd_b
        if not (self.pack_dec_late and not self.merge_packs and self.pack_dec.recs):
            return False
        pkd = Plan("pack_dec")
        with pkd.side(self.LANE_PACK_DEC):
            self.pack_dec.emit(pkd, "pack weights (decoder)")
        fb.splice(1 if (fb.labels and fb.labels[0] == "vq.ema") else 0, pkd, TAG_PACK)
        return True

    def _cut_plans(self):
        """The cuts of fwd_b and bwd a data-parallel caller runs in their place (the same op records: _sub_plan)."""
        fb, bw, ps = self.fwd_b, self.bwd, self.ps
        span = lambda a, b: (lambda i, lab: a <= i < b)
        # Deferred EMA: the EMA accumulators are not read again before the codebook refresh, so the cross-rank sum of
        # z_sum | n_sum can run asynchronously under the whole decoder forward + backward; fwd_b_noema / ema_plan are
        # fwd_b without / only its leading vq.ema op
        self.fwd_b_noema, self.ema_plan = None, None
        if fb.labels and fb.labels[0] == "vq.ema":
            self.fwd_b_noema, self.ema_plan = self._sub_plan("fwd_b_noema", fb, span(1, len(fb.ops))), self._sub_plan("ema", fb, span(0, 1))
        # The same ops as two plans, cut after the decoder's gradients are final: lets a data-parallel
        # caller start reducing the decoder gradients (the contiguous tail of the flat buffer) while the
        # bottleneck / encoder backward still runs (dp.DataParallel.backward_allreduce)
        cut = bw.labels.index("unpack grads (decoder)") + 1 if "unpack grads (decoder)" in bw.labels else len(bw.ops)
        self.bwd_a, self.bwd_b = self._sub_plan("bwd_a", bw, span(0, cut)), self._sub_plan("bwd_b", bw, span(cut, len(bw.ops)))
        # ... and, with the stack's weight gradients as two grouped launches (wgrad_group < layers, e.g. AEW_WGRAD_GROUP=10),
        # bwd_a itself in two: after bwd_a1 every gradient from layer `hi_first_layer` up (+ the post network: the tail of
        # the flat buffer from dec_hi_offset) is final, so that exchange starts under the second half of the chain
        self.bwd_a1 = self.bwd_a2 = None
        self.dec_hi_offset = None
        hi = self.dec.hi_first_layer
        lab_hi = "unpack grads (decoder, upper layers)"
        if hi is not None and lab_hi in bw.labels[:cut]:
            c1 = bw.labels.index(lab_hi) + 1
            self.bwd_a1, self.bwd_a2 = self._sub_plan("bwd_a1", bw, span(0, c1)), self._sub_plan("bwd_a2", bw, span(c1, cut))
            self.dec_hi_offset = min(ps.off[n] for n in ps.names() if n.startswith(self.dec.pre + f"conv_layers.{hi}."))
            later = [n for n in ps.names() if ps.off[n] >= self.dec_hi_offset]
            assert all(n.startswith(self.dec.pre + "post") or
                       (n.startswith(self.dec.pre + "conv_layers.") and int(n[len(self.dec.pre) + 12:].split(".")[0]) >= hi)
                       for n in later), "layers >= hi and the post network form the tail of the flat buffer"
        dec_names = [n for n in ps.names() if n.startswith(self.dec.pre)]
        self.dec_grad_offset = min(ps.off[n] for n in dec_names)
        assert all(ps.off[n] >= self.dec_grad_offset for n in dec_names) and \
            all(ps.off[n] < self.dec_grad_offset for n in ps.names() if n not in dec_names), "decoder params form the tail"

    def _place_packs(self, dec_packed: bool):
        """The weight-layout packs go first in fwd_a (their tables are complete only now)."""
        pk_plan = Plan("pack")
        if self.merge_packs:
            # every weight layout of the step in ONE table launch at the head of fwd_a (serial plans: three launches fewer)
            allp = CopyTableBuilder(self.ws, "tbl.pack_all")
            for tb in (self.pack_first, self.pack_tbl, self.pack_dec, self.pack_late):
                if tb is not None:
                    allp.recs.extend(tb.recs)
            allp.emit(pk_plan, "pack weights (all layouts)")
        else:
            if not dec_packed:
                with pk_plan.side(self.LANE_PACK_DEC):         # joined by the end of fwd_a
                    self.pack_dec.emit(pk_plan, "pack weights (decoder)")
            if self.pack_first is not None and self.pack_first.recs:
                self.pack_first.emit(pk_plan, "pack weights (encoder layer 0)")
                with pk_plan.side(self.PACK_LANE):
                    self.pack_tbl.emit(pk_plan, "pack weights")
            else:
                self.pack_tbl.emit(pk_plan, "pack weights")
        self.fwd_a.splice(0, pk_plan, TAG_PACK)

    def _build_optimizer(self):
        """opt, clip and ratio: one op each, re-addressed per call by adam_step / grad_norm_step / ratio_step."""
        ws, ps = self.ws, self.ps
        self.opt = Plan("adam")
        self.adam_m = ws.alloc("adam.m", ps.numel, torch.float32)
        self.adam_v = ws.alloc("adam.v", ps.numel, torch.float32)
        ad = L.Adam()
        ad.p, ad.g, ad.m, ad.v = ps.params.data_ptr(), ps.grads.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr()
        ad.n = ps.numel
        ad.lr, ad.beta1, ad.beta2, ad.eps, ad.bc1, ad.bc2, ad.grad_scale = 1e-4, 0.9, 0.999, 1e-8, 1.0, 1.0, 1.0
        ad.guard = self.chain_guard.data_ptr()
        self.opt.add(L.OP_ADAM, ad, "adam", TAG_ADAM)
        # ===== global-norm gradient clipping (a plan of its own; runs only when adam_step() is given max_grad_norm)
        self.clip = Plan("clip")
        gn = L.GradNorm()
        gn.x[0], gn.n[0], gn.n_ranges, gn.finalize = ps.grads.data_ptr(), ps.numel, 1, 1
        gn.max_norm, gn.grad_scale, gn.eps = 1.0, 1.0, 1e-6
        # any cut of [0, numel) into <= 8 ranges has at most this many chunks (aew_grad_norm_size)
        self.clip_scratch = ws.alloc("clip.scratch", ps.numel // L.GRAD_NORM_CHUNK + 1 + L.GRAD_NORM_MAX_RANGES, torch.float64)
        self.clip_ticket = ws.alloc("clip.ticket", 4, torch.int32)
        self.clip_sumsq = ws.alloc("clip.sumsq", 2, torch.float64)     # [0] the total; [1] a sharded caller's partial sum
        self.clip_out = ws.alloc("clip.out", 4, torch.float32)         # norm, coefficient, non-finite flag, steps skipped
        gn.sumsq, gn.out = self.clip_sumsq.data_ptr(), self.clip_out.data_ptr()
        gn.scratch, gn.ticket = self.clip_scratch.data_ptr(), self.clip_ticket.data_ptr()
        gn.guard = self.chain_guard.data_ptr()
        self.clip.add(L.OP_GRAD_NORM, gn, "grad norm", TAG_ADAM)
        # ===== per-parameter update / weight ratios (aew_uw_track_t: runs only when adam_step() is given track=True)
        names = ps.names()
        chunks, first = L.uw_chunks([ps.off[n] for n in names], [ps.numel_of(n) for n in names])
        P, nch = len(names), first[-1]
        self.uw_n, self.uw_first_host, self._uw_chunks_host = P, first, chunks
        self.uw_chunks = ws.alloc("uw.chunks", 2 * nch, torch.int64)          # aew_uw_chunk_t records (16 bytes each)
        self.uw_chunks[:2 * nch].copy_(torch.frombuffer(bytearray(bytes(chunks))[:16 * nch], dtype=torch.int64))
        self.uw_first = ws.alloc("uw.first", P + 1, torch.int32)
        self.uw_first[:P + 1].copy_(torch.tensor(first, dtype=torch.int32))
        self.uw_part = ws.alloc("uw.part", 2 * nch, torch.float64)            # per chunk: sum (p_old - p_new)^2, sum p_old^2
        self.uw_sums = ws.alloc("uw.sums", 2 * P, torch.float64)              # per tensor, [2][P]
        self.uw_out = ws.alloc("uw.out", 3 * P, torch.float32)                # [3][P]: update norm, weight norm, ratio
        tr = self.uw_track = L.UwTrack()                                      # host record; the Adam op holds its address
        tr.chunks, tr.chunks_host, tr.n_chunks = self.uw_chunks.data_ptr(), C.addressof(chunks), nch
        tr.part = self.uw_part.data_ptr()
        self._uw_zero, self._uw_stale = True, False
        # ===== parameter groups (aew_adam_groups_t: runs only when adam_step() is given groups): the same chunk table;
        # the device table of P tensor records exists from the first grouped step on (_groups_table)
        gr = self.adam_groups = L.AdamGroups()                                # host record; the grouped Adam op holds its address
        gr.chunks, gr.chunks_host, gr.n_chunks, gr.n_tensors = self.uw_chunks.data_ptr(), C.addressof(chunks), nch, P
        self._tensor_span = [(ps.off[n], ps.off[n] + ru(ps.numel_of(n), 4)) for n in names]   # pad elements included
        self.ratio = Plan("ratio")
        ur = L.UpdateRatio()
        ur.part, ur.first, ur.n_tensors, ur.finalize = self.uw_part.data_ptr(), self.uw_first.data_ptr(), P, 1
        ur.sums, ur.out = self.uw_sums.data_ptr(), self.uw_out.data_ptr()
        self.ratio.add(L.OP_UPDATE_RATIO, ur, "update ratio", TAG_ADAM)

    def _declare_lazy(self):
        """The state that later methods complete at its first use: declared here, empty."""
        self._ema_work = None             # a deferred EMA exchange in flight (forward / finish_ema)
        # ===== averaged (EMA) weights (aew_adam_t.avg: updated only when adam_step() is given avg_rate) and the swap
        # that puts them in the parameters' place for sampling / evaluation
        self.adam_avg = None              # flat like adam_m / adam_v; allocated by the first use (_avg_buffer): an engine that
                                          # never averages holds neither the 4 bytes per parameter nor the swap op
        self.avg_steps = 0                # averaged steps taken so far (a skipped step counts, like step_count)
        self.avg_live = False             # adam_avg holds an average (started by a step, or restored by load_opt_state)
        self.averaged_in = False          # the average sits in ps.params, the raw parameters in adam_avg
        self.swap = Plan("swap")          # one op over ps.params / adam_avg, added with the buffer
        # ===== parameter groups: the device table of tensor records, what it holds and the pinned ring it is sent through
        self.adam_groups_tbl = None       # int32 [P][4] (aew_adam_tensor_t); allocated by the first grouped step
        self.opt_groups = Plan("adam groups")   # one AEW_OP_ADAM_GROUPS op, added with the table
        self._groups_sent = None          # the bytes the table holds (an upload happens only when they change)
        self._groups_ring = None
        # ===== restart of dead codes (aew_vq_restart_t, vqvae-ema only): like the average, the counters, the pair list
        # and the op exist from the first restart_codes() on
        self.restart = Plan("restart")    # one op over bn.lin / emb / ema_numer / ema_denom, added with its buffers
        self.restart_buf = None           # int32 [4]: dead, restarted, total restarted, 0 (restart_out())
        self.restart_pairs_buf = None     # int32 [AEW_VQ_RESTART_MAX][2]: (code, row) per restart (restart_pairs())
        self.lin_live = False             # a forward (or encode) of this engine has filled bn.lin
        # ===== held-out evaluation (evaluate() / aew_eval_acc_t): like the restart, its buffers and plans exist from the
        # first use on (eval_plans())
        self.act_epoch = 0                # bumped by everything that overwrites the activations a backward reads
        self.eval_a = self.eval_b = self.eval_fin = None      # the forward plans minus EVAL_DROP (+ loss, accumulate); finalize
        self.eval_acc = self.eval_hist = self.eval_out = self.eval_loss = None
        # ===== evaluation by group (aew_eval_groups_t): the per-group record, the (group, code) table and the two plans
        # exist from the first grouped evaluation on (eval_group_plans()); an engine that never groups holds none of them
        self.eval_G = 0                   # number of groups the record was built for
        self.eval_grouping = False        # evaluate() also folds the batch into the grouped record (in.group)
        self.eval_g = self.eval_gfin = None
        self.eval_gacc = self.eval_ghist = self.eval_gtot = self.eval_win = self.eval_gout = self.eval_tout = None
        self.in_group = None              # int64 [B]: the group id per window of the batch evaluate() folds
        # ===== gradient accumulation (aew_accum_t): the running sums of a group of micro-batches and the op that folds
        # into them exist from the first micro-step of an engine used with accumulate > 1 (accum_grads / accum_stats)
        self.acc_grads = None             # flat like ps.grads: the sum of the open group's gradients
        self.acc_stats = None             # vqvae-ema: z_sum | n_sum of the open group, laid out like bn.zn_sum
        self.accum = Plan("accum")        # one op, re-addressed per call like `opt` (the mode is a scalar of the op)
        # ===== the encode / conditioning sub-plans (encode(), conditioning()) and the chained launches' host-side watch
        self._encode_plan = self._cond_plan = self._cond_plan_a = None
        # ===== codes as an interface (encode_codes() / codes_to_conditioning()): the lookup op in front of the
        # conditioning plan and the word that counts codes outside the codebook exist from the first decode on
        self._decode_plan = None          # [code.lookup] + the ops of _cond_plan
        self.codes_bad = None             # int32 [1] (a uint32 count): codes outside [0, K) in the last decode
        # ===== whole utterances (encode_tiles(): aew_mel_tile_t / aew_code_stitch_t): one op each in front of and behind
        # _cond_plan_a, re-addressed per batch like `opt`; they exist from the first whole-utterance encode on
        self.utt_tile, self.utt_stitch = Plan("utt.tile"), Plan("utt.stitch")
        # ===== whole utterances, the decoder's side (conditioning_tiles(): aew_code_tile_t / aew_cond_stitch_t): one op each
        # in front of and behind the decode plan, re-addressed per batch in the same way
        self.cond_tile, self.cond_stitch = Plan("code.tile"), Plan("cond.stitch")
        self._dec_pack_plan = None        # decoder_pack_plan(): the decoder's weight layouts alone
        # ===== whole utterances through the teacher-forced decoder (score_tiles(): aew_wav_tile_t / aew_nll_stitch_t /
        # aew_score_reduce_t): one op each around score_plan(), re-addressed per call; they exist from the first scoring on
        self.score_tile, self.score_stitch, self.score_reduce = Plan("wav.tile"), Plan("nll.stitch"), Plan("score.reduce")
        self._score_plan = self._score_dec_plan = None    # decode_plan() + eval_b from the first gated layer through softmax_nll
        self.score_bad = None             # int32 [1] (a uint32 count): samples outside [0, n_quant) in the last scoring
        self._chain_flag_views = self._chain_host = None

    # ops of the training forward that an evaluation leaves out: they write what the next training step (or the caller,
    # through objective.metrics) reads - the EMA statistics and accumulators, the index histogram, the diagnostics, the
    # loss word - or serve the backward alone
    EVAL_DROP = ("vq.stats", "n_sum -> diagnostics copy", "vq.ema", "pack weights (backward layouts)",
                 "diagnostics (codebook)", "diagnostics (peak)", "metrics", "loss")

    def eval_plans(self):
        """Held-out evaluation, built once at its first use: the forward plans without EVAL_DROP (the same op records,
        order, lanes and chained launches), the loss reduction once more into a word of its own, and the accumulator
        (aew_eval_acc_t) that folds the batch into the running record eval_acc (float64 [16]) / eval_hist (uint32 [K],
        held as int32).  eval_fin turns the record into eval_out.  Returns (eval_a, eval_b, eval_fin)."""
        if self.eval_fin is not None:
            return self.eval_a, self.eval_b, self.eval_fin
        ws, fb = self.ws, self.fwd_b
        K = self.bn.K if self.bn is not None else 0
        self.eval_acc = ws.alloc("eval.acc", L.EVAL_ACC_N, torch.float64)[:L.EVAL_ACC_N]
        self.eval_hist = ws.alloc("eval.hist", max(K, 1), torch.int32)[:max(K, 1)]     # (uint32 counts)
        self.eval_out = ws.alloc("eval.out", L.EVAL_OUT_N, torch.float32)[:L.EVAL_OUT_N]
        self.eval_loss = ws.alloc("eval.loss", 8, torch.float32)
        keep = lambda i, lab: lab not in self.EVAL_DROP
        self.eval_a = self._sub_plan("eval_a", self.fwd_a, keep)
        self.eval_b = self._sub_plan("eval_b", fb, keep)
        red = L.Reduce.from_buffer_copy(fb.ops[fb.labels.index("loss")].u.red)     # the same terms (and device-side anneal weight)
        red.out = self.eval_loss.data_ptr()
        self.eval_b.add(L.OP_REDUCE, red, "eval.loss", TAG_LOSS)
        sm = fb.ops[fb.labels.index("softmax_nll")].u.sm
        ev = L.EvalAcc()
        ev.nll, ev.ptgt, ev.wav, ev.wav_pitch, ev.tgt_off, ev.B, ev.w = sm.nll, sm.ptgt, sm.wav, sm.wav_pitch, sm.tgt_off, sm.B, sm.w
        if sm.amax:
            ev.amax = sm.amax
        else:
            ev.logits, ev.bs, ev.pitch, ev.n_quant = sm.logits, sm.bs, sm.pitch, sm.Q
        if K:
            ev.ind, ev.dist, ev.Q, ev.K = self.ind.data_ptr(), self.min_dist.data_ptr(), self.Q, K
            ev.hist = self.eval_hist.data_ptr()
        ev.loss, ev.acc, ev.out = self.eval_loss.data_ptr(), self.eval_acc.data_ptr(), self.eval_out.data_ptr()
        self.eval_b.add(L.OP_EVAL_ACC, ev, "eval.accumulate", TAG_LOSS)
        fin = L.EvalAcc.from_buffer_copy(ev)
        fin.finalize = 1
        self.eval_fin = Plan("eval_fin")
        self.eval_fin.add(L.OP_EVAL_ACC, fin, "eval.finalize", TAG_LOSS)
        return self.eval_a, self.eval_b, self.eval_fin

    def eval_group_plans(self, G: int):
        """Evaluation by group, built once at its first use: the record of aew_eval_groups_t for G groups - eval_gacc
        (float64 [G][8]), eval_ghist (uint32 [G][K] held as int32; absent without a codebook), eval_gtot (float64 [4]),
        eval_win (float64 [B][4]) -, the outputs eval_gout (float [G][12]) / eval_tout (float [16]), the group ids
        in_group (int64 [B]) and two one-op plans: eval_g folds the batch evaluate() just ran (its pointers are those of
        the softmax_nll op, as eval.accumulate's), eval_gfin turns the record into the outputs.  The plain evaluation
        plans are not touched.  Returns (eval_g, eval_gfin)."""
        G = int(G)
        if self.eval_gfin is not None and G == self.eval_G:
            return self.eval_g, self.eval_gfin
        if G < 1:
            raise L.AewError(f"evaluation by group needs at least one group, got {G}")
        if self.eval_gfin is not None:             # another number of groups: the record and its two plans are built anew
            for name in ("eval.gacc", "eval.ghist", "eval.gscratch", "eval.gtot", "eval.win", "eval.gout", "eval.tout", "in.group"):
                self.ws.bufs.pop(name, None)
            self.eval_ghist = None
        self.eval_plans()
        ws, fb, B = self.ws, self.fwd_b, self.B
        K = self.bn.K if self.bn is not None else 0
        self.eval_gacc = ws.alloc("eval.gacc", G * L.EVAL_GACC_N, torch.float64)[:G * L.EVAL_GACC_N].view(G, L.EVAL_GACC_N)
        if K:
            self.eval_ghist = ws.alloc("eval.ghist", G * K, torch.int32)[:G * K].view(G, K)     # (uint32 counts)
            scratch = ws.alloc("eval.gscratch", K + 4 * G, torch.float64)
        self.eval_gtot = ws.alloc("eval.gtot", 4, torch.float64)[:4]
        self.eval_win = ws.alloc("eval.win", B * 4, torch.float64)[:B * 4].view(B, 4)
        self.eval_gout = ws.alloc("eval.gout", G * L.EVAL_GOUT_N, torch.float32)[:G * L.EVAL_GOUT_N].view(G, L.EVAL_GOUT_N)
        self.eval_tout = ws.alloc("eval.tout", L.EVAL_TOUT_N, torch.float32)[:L.EVAL_TOUT_N]
        self.in_group = ws.alloc("in.group", B, torch.int64)[:B]
        sm = fb.ops[fb.labels.index("softmax_nll")].u.sm
        ev = L.EvalGroups()
        ev.nll, ev.ptgt, ev.wav, ev.wav_pitch, ev.tgt_off, ev.B, ev.w = sm.nll, sm.ptgt, sm.wav, sm.wav_pitch, sm.tgt_off, sm.B, sm.w
        if sm.amax:
            ev.amax = sm.amax
        else:
            ev.logits, ev.bs, ev.pitch, ev.n_quant = sm.logits, sm.bs, sm.pitch, sm.Q
        if K:
            ev.ind, ev.dist, ev.Qw, ev.K = self.ind.data_ptr(), self.min_dist.data_ptr(), self.Q // B, K
            ev.ghist, ev.scratch = self.eval_ghist.data_ptr(), scratch.data_ptr()
        ev.group, ev.G = self.in_group.data_ptr(), G
        ev.gacc, ev.gtot, ev.win = self.eval_gacc.data_ptr(), self.eval_gtot.data_ptr(), self.eval_win.data_ptr()
        ev.gout, ev.tout = self.eval_gout.data_ptr(), self.eval_tout.data_ptr()
        self.eval_g = Plan("eval_g")
        self.eval_g.add(L.OP_EVAL_GROUPS, ev, "eval.group_accumulate", TAG_LOSS)
        fin = L.EvalGroups.from_buffer_copy(ev)
        fin.finalize = 1
        self.eval_gfin = Plan("eval_gfin")
        self.eval_gfin.add(L.OP_EVAL_GROUPS, fin, "eval.group_finalize", TAG_LOSS)
        self.eval_G = G
        return self.eval_g, self.eval_gfin

    # --------------------------------------------------------------------------------------
    # execution
    # --------------------------------------------------------------------------------------
    def _stream(self) -> int:
        if self.device.type == "cuda":
            return torch.cuda.current_stream(self.device).cuda_stream
        raise L.AewError("the HIP plans can only run on a GPU device; this engine was built on "
                         f"'{self.device}' (plan construction only)")

    def set_inputs(self, wav, mel, voice, jitter, eps=None):
        g = self.geom
        self.in_wav.copy_(wav)
        self.in_mel.copy_(mel)
        self.in_voice.copy_(voice)
        self.in_jitter.copy_(jitter[:, :g.embed_len])
        if self.bn is not None and self.bn.eps is not None:          # (vae: the noise of the sample)
            if eps is None:
                self.eps.normal_()
            else:
                self.eps.copy_(eps.permute(0, 2, 1) if eps.shape[1] == self.d and eps.dim() == 3 else eps)

    def set_anneal_weight(self, a: float):
        """SGVBLoss.update_anneal_weight (vae_bn.py:72-73).  The weight changes every step
        (chassis.py:148-149), so the ops read it from device memory (`anneal_buf`): no descriptor is
        patched and no captured graph is invalidated."""
        self.anneal_weight = float(a)
        self.bn.anneal_buf.fill_(float(a))
        # Data parallel (dp.DataParallel): the optimizer scales the SUMMED gradient by 1/world (mean-type NLL), but
        # the KL term is a sum over all windows of the global batch, so its gradient must not be divided: pre-multiply
        self.bn.anneal_bwd.fill_(float(a) * float(self.dp_world))

    def _run(self, plan, timing=False):
        # self.tuning: an aew_tuning_t of this engine's own (None: the process-wide switches).  Note that plan
        # CONSTRUCTION (split-K slab counts) always follows the process-wide record.
        if self.use_graphs and not timing:
            tun = self.tuning
            if self.graph_lanes and plan._graph is None and any(op.lane >= 4 for op in plan.ops):
                # capture: lanes 4 / 5 (DecoderPlan.tail_lane: the last grouped weight-gradient launch as a branch beside
                # the rest of the backward) become graph branches unless the caller chose a lane mode itself
                tun = L.current_tuning() if tun is None else L.Tuning.from_buffer_copy(tun)
                if tun.lanes == 0:
                    tun.lanes = self.graph_lanes
            plan.run_graph(self._stream(), tuning=tun)
        else:
            plan.run(self._stream(), tuning=self.tuning)

    def _sub_plan(self, name: str, src: Plan, keep) -> Plan:
        """A plan made of the ops of `src` whose (index, label) passes `keep` (shares the op records)."""
        sp = Plan(name)
        idx = [i for i, lab in enumerate(src.labels) if keep(i, lab)]
        sp.ops, sp.labels = [src.ops[i] for i in idx], [src.labels[i] for i in idx]
        return sp

    def encode(self):
        """Encoder + bottleneck.linear only (what autoencoder_model.py:171-199 runs to collect k-means samples):
        no nearest-code search, no EMA statistics, no index histogram update.  Result in `self.lin`."""
        if self._encode_plan is None:
            fa = self.fwd_a
            stop = fa.labels.index("bn.linear") + 1
            self._encode_plan = self._sub_plan("encode", fa, lambda i, lab: i < stop)
        self._run(self._encode_plan, False)
        self.lin_live = True

    def _cond_plans(self):
        """The two halves of conditioning(), built once: _cond_plan_a = fwd_a without vq.stats (encoder, bn.linear, nearest
        code), _cond_plan = the prefix of fwd_b in front of the first gated layer, without vq.ema and the chained launches."""
        if self._cond_plan is None:
            fb = self.fwd_b
            stop = fb.labels.index("G1.0") if "G1.0" in fb.labels else next(
                i for i, l in enumerate(fb.labels) if l.startswith("G1.0"))
            self._cond_plan = self._sub_plan("conditioning", fb, lambda i, lab: i < stop and lab != "vq.ema" and
                                             not lab.startswith("chain["))
            self._cond_plan_a = self._sub_plan("conditioning_a", self.fwd_a, lambda i, lab: lab != "vq.stats")

    def _cond_out(self):
        d = self.dec
        return d.cond.tensor(), d.bias_bl[:self.B * d.NL * 2 * d.Dp].view(self.B, d.NL, 2 * d.Dp)

    def _need_codes(self, what: str):
        if not hasattr(self.bn, "lookup_op"):
            raise L.AewError(f"{what} needs a VQ bottleneck (vqvae or vqvae-ema): the bottleneck of this engine is "
                             f"'{self.bn_type}', which has no discrete codes")

    def encode_codes(self):
        """Encoder -> bn.linear -> nearest code for the batch in the inputs (_cond_plan_a: the training forward's first half
        without vq.stats): the codes are left in `ind` [Q = B * embed_len], their distances in `min_dist`.  Writes no
        EMA statistic, histogram, loss or metric word; overwrites the encoder activations (act_epoch).  No host
        synchronisation.  Returns (ind, min_dist) as views of the workspace buffers."""
        self._need_codes("encode_codes()")
        self._cond_plans()
        self.act_epoch += 1
        self._run(self._cond_plan_a, False)
        self.lin_live = True
        return self.ind[:self.Q], self.min_dist[:self.Q]

    def utterance_ops(self):
        """The records of the two ops around _cond_plan_a in a whole-utterance encode, built at the first use:
        (aew_mel_tile_t writing in_mel, aew_code_stitch_t reading ind / min_dist).  The caller fills in the table, its
        first row, the ragged buffers and their sizes."""
        self._need_codes("encode_tiles()")
        if not self.utt_tile.ops:
            g = self.geom
            E, _, _, mel_len = G.utterance_geometry(g)
            mt = L.MelTile()
            mt.in_mel, mt.B, mt.n_mel, mt.mel_len = self.in_mel.data_ptr(), self.B, self.n_mel, mel_len
            self.utt_tile.add(L.OP_MEL_TILE, mt, "utt.tile", TAG_VQ)
            cs = L.CodeStitch()
            cs.ind, cs.min_dist, cs.B, cs.E = self.ind.data_ptr(), self.min_dist.data_ptr(), self.B, E
            self.utt_stitch.add(L.OP_CODE_STITCH, cs, "utt.stitch", TAG_VQ)
        return self.utt_tile.array()[0].u.mtile, self.utt_stitch.array()[0].u.cstitch

    # ---- whole utterances in tiles: the path encode / segment / conditioning / score share ---------------------------------
    @staticmethod
    def _tile_rec(plan: Plan):
        """The record of a one-op plan, as the plan runs it (a view into plan.array())."""
        op = plan.array()[0]
        return getattr(op.u, L.OP_FIELD[op.kind])

    @staticmethod
    def _tile_fill(recs, fields, table: int, table_host: int, first_row: int = 0):
        """The table's two addresses and a first row on the tile and the stitch record, then each one's own `fields`."""
        for rec, own in zip(recs, fields):
            rec.table, rec.table_host, rec.first_row = table, table_host, first_row
            for name, value in own.items():
                setattr(rec, name, value)

    def _tile_rows(self, what: str, table, row, c_name: str) -> int:
        """len(table), or raises unless it holds a multiple of B records of the struct `row`."""
        n = len(table)
        if n % self.B or table.dtype.itemsize != C.sizeof(row):
            raise L.AewError(f"{what}: a multiple of B = {self.B} {c_name} records expected, got {n}")
        return n

    def _run_tiles(self, tile: Plan, body: Plan, stitch: Plan, fields, table, extra=()):
        """`table` (a checked numpy array of row records) - and the bytes of the arrays `extra` behind it - go to the device
        once (plan.pinned_upload); then per batch of B rows: the one-op plan `tile`, the engine's `body` unchanged, the
        one-op plan `stitch`.  fields = (the tile record's own fields, the stitch record's).  The host sets first_row and
        runs three plans per batch, nothing else.  Whatever happens, both records end as they were built: they keep no
        address of the caller's tensors nor of the table, which returns to torch's allocators - those order its reuse
        behind this stream's work.  -> (device bytes, pinned host bytes) of table + extra."""
        dev, host = pinned_upload(self.device, table, *extra)
        n, recs = len(table), (self._tile_rec(tile), self._tile_rec(stitch))
        built = [bytes(r) for r in recs]
        try:
            self._tile_fill(recs, fields, dev.data_ptr(), host.data_ptr())
            st = self._stream()
            for first in range(0, n, self.B):
                recs[0].first_row = recs[1].first_row = first
                tile.run(st)
                self._run(body, False)
                stitch.run(st)
        finally:
            for rec, was in zip(recs, built):
                C.memmove(C.addressof(rec), was, len(was))
        return dev, host

    def _tile_batch_plan(self, name: str, tile: Plan, body: Plan, stitch: Plan, fields, table: torch.Tensor,
                         table_host: torch.Tensor, first_row: int, join: bool = False) -> Plan:
        """[tile] + the ops of `body` (the same records) + [stitch] as one plan for a caller's captured graph: copies of
        the two records, filled as _run_tiles() fills them, over the rows [first_row, first_row + B) of `table`."""
        recs = [type(r).from_buffer_copy(r) for r in (self._tile_rec(tile), self._tile_rec(stitch))]
        self._tile_fill(recs, fields, table.data_ptr(), table_host.data_ptr(), int(first_row))
        p = Plan(name)
        p.add(tile.ops[0].kind, recs[0], tile.labels[0], tile.ops[0].tag)
        p.splice(1, self._sub_plan(body.name, body, lambda i, lab: True))
        p.add(stitch.ops[0].kind, recs[1], stitch.labels[0], stitch.ops[0].tag, join=join)
        return p

    @staticmethod
    def _utt_fields(mel, codes=None, dist=None):
        return (dict(mel=mel.data_ptr(), n_src=mel.numel()),
                {} if codes is None else dict(codes=codes.data_ptr(), n_dst=codes.numel(),
                                              dist=dist.data_ptr() if dist is not None else None))

    def utterance_batch_plan(self, mel: torch.Tensor, table: torch.Tensor, table_host: torch.Tensor, first_row: int,
                             codes: torch.Tensor, dist: Optional[torch.Tensor] = None) -> Plan:
        """One batch of a whole-utterance encode as a plan of its own (for a caller's captured graph): [utt.tile] + the
        ops of _cond_plan_a (the same records) + [utt.stitch] over the rows [first_row, first_row + B) of `table` (uint8
        device bytes of aew_utt_row_t records; table_host: the same bytes in pinned host memory, read at capture).  The
        caller keeps the tensors alive."""
        self.utterance_ops()
        self._cond_plans()
        return self._tile_batch_plan("utt.batch", self.utt_tile, self._cond_plan_a, self.utt_stitch,
                                     self._utt_fields(mel, codes, dist), table, table_host, first_row)

    def encode_tiles(self, mel: torch.Tensor, table, codes: torch.Tensor, dist: Optional[torch.Tensor] = None):
        """Whole utterances through the fixed-geometry encoder: `mel` flat fp32, the ragged buffer of the utterances'
        (n_mel, F_u) arrays; `table` a numpy array of aew_utt_row_t records (_lib.UTT_ROW_DTYPE), a multiple of B rows
        (codes.TilePlan.table); `codes` int64 - and `dist` fp32 - flat outputs.  The table goes to the device once (pinned,
        non-blocking); per batch of B rows one AEW_OP_MEL_TILE fills in_mel, _cond_plan_a runs unchanged and one
        AEW_OP_CODE_STITCH moves the codes whose receptive field lies inside real frames (_run_tiles).  Writes what
        encode_codes() writes and nothing else of the engine; no host synchronisation."""
        self.utterance_ops()
        self._cond_plans()
        n = self._tile_rows("encode_tiles()", table, L.UttRow, "aew_utt_row_t")
        if mel.dtype != torch.float32 or codes.dtype != torch.int64 or not mel.is_contiguous() or not codes.is_contiguous() \
                or (dist is not None and (dist.dtype != torch.float32 or dist.numel() != codes.numel())):
            raise L.AewError("encode_tiles(): flat fp32 mel, int64 codes and fp32 dist (one per code) expected")
        if n == 0:
            return
        self.act_epoch += 1
        self._run_tiles(self.utt_tile, self._cond_plan_a, self.utt_stitch, self._utt_fields(mel, codes, dist), table)
        self.lin_live = True

    def segment_tiles(self, mel: torch.Tensor, table, offsets, penalty, return_dist: bool = False):
        """Whole utterances through the fixed-geometry encoder and a penalised Viterbi pass over the codebook: `mel`, `table`
        as in encode_tiles(); `offsets` (U + 1,) host integers, the codes each utterance owns (codes.TilePlan.offsets);
        `penalty` one float or one per utterance.  Per batch of B rows one AEW_OP_MEL_TILE fills in_mel, _cond_plan_a runs
        unchanged and one AEW_OP_FRAME_STITCH moves the encoder outputs (bn.lin rows) whose receptive field lies inside real
        frames to a ragged (n_codes, pitch) buffer (_run_tiles); behind the last batch ONE AEW_OP_CODE_SEGMENT chooses the
        codes of all utterances against the live codebook under the engine's metric (codes.segment_full).  The nearest
        codes of the batches stay in `ind` and are not stitched: they are no output of this call.  Writes what
        encode_tiles() writes and nothing else of the engine; no host synchronisation.
        -> (codes, dist or None, codes.Segmentation)."""
        from . import codes as CD
        self.utterance_ops()
        self._cond_plans()
        bn = self.bn
        n = self._tile_rows("segment_tiles()", table, L.UttRow, "aew_utt_row_t")
        if mel.dtype != torch.float32 or not mel.is_contiguous():
            raise L.AewError("segment_tiles(): flat fp32 mel expected")
        offsets = np.asarray(offsets, np.int64).reshape(-1)
        n_codes = int(offsets[-1])
        frames = torch.empty(n_codes, bn.nlin_p, dtype=torch.float32, device=self.device)
        if n:
            fs = L.FrameStitch()
            fs.B, fs.E, fs.lin, fs.lin_bs, fs.d_pitch = self.B, self.geom.embed_len, bn.lin.ptr, bn.lin.bs, bn.nlin_p
            fs.frames, fs.n_dst = frames.data_ptr(), n_codes
            stitch = Plan("utt.frames")
            stitch.add(L.OP_FRAME_STITCH, fs, "utt.frames", TAG_VQ)
            self.act_epoch += 1
            self._run_tiles(self.utt_tile, self._cond_plan_a, stitch, self._utt_fields(mel), table)
            self.lin_live = True
        emb = self.emb.view(bn.K, bn.d)
        return CD.segment_full(frames, offsets, emb, penalty, CD.VQ_METRIC_NAMES[bn.metric], return_dist)

    DECODE_DROP = ("diagnostics (codebook)",)

    def decode_plan(self) -> Plan:
        """[code.lookup] + the ops of _cond_plan (the same records), built at the first use with the `codes_bad` word.
        One op of _cond_plan is left out: "diagnostics (codebook)" sits in front of the first gated layer on a side lane
        of fwd_b, reduces the ENCODER outputs bn.lin - which a decode never computed - and writes `diag`, the record
        behind objective.metrics.  Nothing the conditioning needs depends on it."""
        self._need_codes("codes_to_conditioning()")
        if self._decode_plan is None:
            self._cond_plans()
            self.codes_bad = self.ws.alloc("codes.bad", 1, torch.int32)
            head = Plan("lookup")
            head.add(L.OP_CODE_LOOKUP, self.bn.lookup_op(self.codes_bad), "code.lookup", TAG_VQ)
            dp = self._sub_plan("codes_to_conditioning", self._cond_plan, lambda i, lab: lab not in self.DECODE_DROP)
            dp.splice(0, head)
            self._decode_plan = dp
        return self._decode_plan

    def codes_to_conditioning(self, codes: torch.Tensor):
        """The decoder's conditioning from GIVEN codes (int64, B * embed_len of them, row-major) instead of the encoder's:
        the codes go to `ind`, one AEW_OP_CODE_LOOKUP writes bn.zq = emb[ind] and the conditioning plan runs unchanged.
        `voice` and `jitter` are read from the inputs (set_inputs / the in_voice, in_jitter buffers).  A code outside
        [0, K) is not followed: its row of zq is zero and `codes_bad[0]` counts it - the caller decides (reading the word
        synchronises).  Writes none of emb, the EMA accumulators and statistics, ind_hist, loss_buf, met_buf, diag, the
        parameters, gradients, moments or the average; overwrites activations (act_epoch).  A deferred EMA accumulation is
        applied first, as evaluate() does: the lookup reads the codebook behind it.
        Returns (cond, bias) exactly as conditioning() does."""
        dp = self.decode_plan()
        if codes.dtype != torch.int64 or codes.numel() != self.Q:
            raise L.AewError(f"codes_to_conditioning(): {self.Q} int64 codes expected (B = {self.B} rows of "
                             f"{self.geom.embed_len}), got {tuple(codes.shape)} {codes.dtype}")
        self.finish_ema()
        self.act_epoch += 1
        self.ind[:self.Q].copy_(codes.reshape(-1))
        self.codes_bad.zero_()
        self._run(dp, False)
        return self._cond_out()

    def conditioning_ops(self):
        """The records of the two ops around the decode plan in a whole-utterance conditioning, built at the first use:
        (aew_code_tile_t writing ind / in_voice and counting into codes_bad, aew_cond_stitch_t reading dec.cond and the
        gated bias).  The caller fills in the table, its first row, the flat codes and the per-stream outputs."""
        self.decode_plan()
        if self.take_compat:
            raise L.AewError("conditioning_tiles(): this engine was built with take_compat=True, whose conditioning gather "
                             "is not the identity the tiling of whole utterances rests on")
        if not self.cond_tile.ops:
            d = self.dec
            G.conditioning_geometry(self.geom)                       # (raises for a window shorter than one hop)
            ct = L.CodeTile()
            ct.ind, ct.in_voice, ct.bad = self.ind.data_ptr(), self.in_voice.data_ptr(), self.codes_bad.data_ptr()
            ct.B, ct.E, ct.K, ct.n_voice = self.B, self.geom.embed_len, self.K, int(self.hps.n_speakers)
            self.cond_tile.add(L.OP_CODE_TILE, ct, "code.tile", TAG_VQ)
            cs = L.CondStitch()
            cs.cond, cs.cond_bs, cs.cond_pitch, cs.T, cs.Cp = d.cond.ptr, d.cond.bs, d.cond.pitch, d.T, d.Cp
            cs.bias, cs.bias_n, cs.B = d.bias_bl.data_ptr(), d.NL * 2 * d.Dp, self.B
            self.cond_stitch.add(L.OP_COND_STITCH, cs, "cond.stitch", TAG_UPS)
        return self.cond_tile.array()[0].u.ctile, self.cond_stitch.array()[0].u.cndst

    def decoder_pack_plan(self) -> Plan:
        """The pack of the decoder's weight layouts as a plan of its own, built at the first use.  The conditioning GEMMs
        read packed copies of the parameters that the training forward refreshes at its head; decode_plan() holds that
        pack only where it sits in fwd_b (separate packs, placed late).  A whole-utterance conditioning may be the first
        thing a process runs - codes from disk, weights from a checkpoint - so it packs for itself: the same op record
        where one exists, else a table of the decoder's records alone (the merged table packs every layout of the step)."""
        if self._dec_pack_plan is None:
            lab = "pack weights (decoder)"
            if lab in self.decode_plan().labels:
                self._dec_pack_plan = Plan("pack_dec")               # (already part of the decode plan: nothing to add)
            elif lab in self.fwd_a.labels:
                op = L.Op.from_buffer_copy(self.fwd_a.ops[self.fwd_a.labels.index(lab)])
                op.lane = op.join = 0                                # (a side-lane op there; alone it is the main lane)
                self._dec_pack_plan = Plan("pack_dec")
                self._dec_pack_plan.ops.append(op)
                self._dec_pack_plan.labels.append(lab)
            else:
                tb = CopyTableBuilder(self.ws, "tbl.pack_dec_alone")
                tb.recs.extend(L.CopyRec.from_buffer_copy(r) for r in self.pack_dec.recs)
                self._dec_pack_plan = Plan("pack_dec")
                tb.emit(self._dec_pack_plan, lab)
        return self._dec_pack_plan

    def _cond_utt_check(self, what: str, codes_flat, cond_utt, bias_utt):
        d = self.dec
        if codes_flat.dtype != torch.int64 or codes_flat.dim() != 1 or not codes_flat.is_contiguous():
            raise L.AewError(f"{what}: flat contiguous int64 codes expected, got {tuple(codes_flat.shape)} {codes_flat.dtype}")
        if cond_utt.dtype != torch.bfloat16 or cond_utt.dim() != 3 or cond_utt.shape[2] != d.Cp or not cond_utt.is_contiguous():
            raise L.AewError(f"{what}: cond_utt bf16 (streams, rows, {d.Cp}) contiguous expected, got {tuple(cond_utt.shape)} "
                             f"{cond_utt.dtype}")
        if bias_utt.dtype != torch.float32 or tuple(bias_utt.shape) != (cond_utt.shape[0], d.NL, 2 * d.Dp) \
                or not bias_utt.is_contiguous():
            raise L.AewError(f"{what}: bias_utt fp32 ({cond_utt.shape[0]}, {d.NL}, {2 * d.Dp}) contiguous expected, got "
                             f"{tuple(bias_utt.shape)} {bias_utt.dtype}")

    @staticmethod
    def _cond_fields(codes_flat, cond_utt, bias_utt):
        return (dict(codes=codes_flat.data_ptr(), n_codes=codes_flat.numel()),
                dict(cond_utt=cond_utt.data_ptr(), n_dst=cond_utt.numel(), bias_utt=bias_utt.data_ptr(), n_streams=cond_utt.shape[0]))

    def conditioning_batch_plan(self, codes_flat: torch.Tensor, table: torch.Tensor, table_host: torch.Tensor, first_row: int,
                                cond_utt: torch.Tensor, bias_utt: torch.Tensor) -> Plan:
        """One batch of a whole-utterance conditioning as a plan of its own (for a caller's captured graph): [code.tile] +
        the ops of decode_plan() (the same records) + [cond.stitch] over the rows [first_row, first_row + B) of `table`
        (uint8 device bytes of aew_cond_row_t records; table_host: the same bytes in pinned host memory, read at
        capture).  in_jitter is set to the identity and the decoder's weight layouts are packed here, once (after a change
        of the weights the caller runs decoder_pack_plan() again); the caller zeroes codes_bad and cond_utt and keeps the
        tensors alive."""
        self.conditioning_ops()
        self._cond_utt_check("conditioning_batch_plan()", codes_flat, cond_utt, bias_utt)
        self.finish_ema()                                            # (a deferred EMA accumulation first, as evaluate())
        self.in_jitter.copy_(torch.arange(self.geom.embed_len, device=self.device).expand(self.B, -1))
        self.decoder_pack_plan().run(self._stream())
        return self._tile_batch_plan("cond.batch", self.cond_tile, self.decode_plan(), self.cond_stitch,
                                     self._cond_fields(codes_flat, cond_utt, bias_utt), table, table_host, first_row)

    def conditioning_tiles(self, codes_flat: torch.Tensor, table, cond_utt: torch.Tensor, bias_utt: torch.Tensor):
        """The conditioning of whole utterances through the fixed-geometry chain: `codes_flat` int64, the flat code
        buffer; `table` a numpy array of aew_cond_row_t records (_lib.COND_ROW_DTYPE), a multiple of B rows
        (codes.CondTilePlan.table); `cond_utt` bf16 (streams, rows per stream, Cp) and `bias_utt` fp32 (streams, NL,
        2 * Dp), contiguous - the caller zero-fills cond_utt once, rows behind an utterance's length are not written.  The
        table goes to the device once (pinned, non-blocking); per batch of B rows one AEW_OP_CODE_TILE fills ind and
        in_voice, decode_plan() runs unchanged with in_jitter the identity, and one AEW_OP_COND_STITCH moves the rows each
        window owns and the gated bias of first windows (_run_tiles).  Codes outside [0, K) become code 0 and count in
        `codes_bad[0]` (zeroed here; non-zero: the caller decides - reading the word synchronises).  Writes what
        codes_to_conditioning() writes, the packed layouts of the decoder's weights (decoder_pack_plan(), once per call:
        what the head of a training forward writes) and nothing else of the engine; no host synchronisation."""
        self.conditioning_ops()
        n = self._tile_rows("conditioning_tiles()", table, L.CondRow, "aew_cond_row_t")
        self._cond_utt_check("conditioning_tiles()", codes_flat, cond_utt, bias_utt)
        self.codes_bad.zero_()
        if n == 0:
            return
        self.finish_ema()                                            # (a deferred EMA accumulation first, as evaluate())
        self.in_jitter.copy_(torch.arange(self.geom.embed_len, device=self.device).expand(self.B, -1))
        self.decoder_pack_plan().run(self._stream())
        self.act_epoch += 1
        self._run_tiles(self.cond_tile, self.decode_plan(), self.cond_stitch, self._cond_fields(codes_flat, cond_utt, bias_utt),
                        table)

    # ---- whole utterances through the teacher-forced decoder: the likelihood of a waveform given codes and a voice ---------
    def score_decoder_plan(self) -> Plan:
        """The decoder half of score_plan(), built once: the ops of eval_b from the first gated layer (its chained launch
        included) through softmax_nll - the same records, order, lanes and chained launches; eval.loss, eval.accumulate
        and everything in EVAL_DROP are left out."""
        if self._score_dec_plan is None:
            eb = self.eval_plans()[1]
            first = next(i for i, lab in enumerate(eb.labels) if lab.startswith(("G1.0", "chain[G1.0")))
            last = eb.labels.index("softmax_nll")
            self._score_dec_plan = self._sub_plan("score_decoder", eb, lambda i, lab: first <= i <= last)
        return self._score_dec_plan

    def score_plan(self) -> Plan:
        """decode_plan() (code lookup + the conditioning prefix with the base gather, the same records) followed by
        score_decoder_plan(), built once at the first use: codes, voices and decoder-input samples in, per-position nll /
        ptgt (and arg-max, where the softmax writes one) out."""
        if self._score_plan is None:
            sp = self._sub_plan("score", self.decode_plan(), lambda i, lab: True)
            sp.splice(len(sp.ops), self._sub_plan("score_decoder", self.score_decoder_plan(), lambda i, lab: True))
            self._score_plan = sp
        return self._score_plan

    def scoring_ops(self):
        """The records of the three ops around the score plan, built at the first use: (aew_wav_tile_t writing in_wav /
        ind / in_voice and counting into codes_bad / score_bad, aew_nll_stitch_t reading what softmax_nll wrote,
        aew_score_reduce_t).  The caller fills in the table, its first row, the flat buffers and the outputs."""
        self.score_plan()
        if self.take_compat:
            raise L.AewError("score_tiles(): this engine was built with take_compat=True, whose conditioning gather is not "
                             "the identity the tiling of whole utterances rests on")
        if not self.score_tile.ops:
            g = self.geom
            G.scoring_geometry(g)                                        # (raises for a window shorter than one hop)
            self.score_bad = self.ws.alloc("score.bad", 1, torch.int32)
            sm = self.fwd_b.ops[self.fwd_b.labels.index("softmax_nll")].u.sm
            wt = L.WavTile()
            wt.ind, wt.in_voice, wt.wav = self.ind.data_ptr(), self.in_voice.data_ptr(), self.in_wav.data_ptr()
            wt.bad_codes, wt.bad_wav = self.codes_bad.data_ptr(), self.score_bad.data_ptr()
            wt.wav_pitch, wt.wav_off, wt.T, wt.n_quant = self.in_wav.shape[1], g.trim_dec_in[0], g.dec_in_len, int(self.hps.n_quant)
            wt.B, wt.E, wt.K, wt.n_voice = self.B, g.embed_len, self.K, int(self.hps.n_speakers)
            from .codes import mu_encode
            wt.zero = float(mu_encode(torch.zeros(1), int(self.hps.n_quant))[0])
            self.score_tile.add(L.OP_WAV_TILE, wt, "wav.tile", TAG_VQ)
            ns = L.NllStitch()
            ns.nll, ns.ptgt, ns.wav, ns.wav_pitch, ns.tgt_off, ns.B, ns.w = sm.nll, sm.ptgt, sm.wav, sm.wav_pitch, sm.tgt_off, sm.B, sm.w
            if sm.amax:
                ns.amax = sm.amax
            else:
                ns.logits, ns.bs, ns.pitch, ns.n_quant = sm.logits, sm.bs, sm.pitch, sm.Q
            self.score_stitch.add(L.OP_NLL_STITCH, ns, "nll.stitch", TAG_LOSS)
            self.score_reduce.add(L.OP_SCORE_REDUCE, L.ScoreReduce(), "score.reduce", TAG_LOSS)
        return self.score_tile.array()[0].u.wtile, self.score_stitch.array()[0].u.nllst, self.score_reduce.array()[0].u.sred

    def _score_check(self, what: str, codes_flat, wav_flat, nll, ptgt, hit):
        if codes_flat.dtype != torch.int64 or codes_flat.dim() != 1 or not codes_flat.is_contiguous():
            raise L.AewError(f"{what}: flat contiguous int64 codes expected, got {tuple(codes_flat.shape)} {codes_flat.dtype}")
        if wav_flat.dtype != torch.float32 or wav_flat.dim() != 1 or not wav_flat.is_contiguous():
            raise L.AewError(f"{what}: a flat contiguous float32 waveform buffer expected, got {tuple(wav_flat.shape)} "
                             f"{wav_flat.dtype}")
        if nll.dtype != torch.float32 or nll.dim() != 1 or not nll.is_contiguous():
            raise L.AewError(f"{what}: flat contiguous float32 nll expected, got {tuple(nll.shape)} {nll.dtype}")
        for name, t, dt in (("ptgt", ptgt, torch.float32), ("hit", hit, torch.uint8)):
            if t is not None and (t.dtype != dt or t.shape != nll.shape or not t.is_contiguous()):
                raise L.AewError(f"{what}: {name} must be {dt}, contiguous, one value per nll element")

    @staticmethod
    def _score_fields(codes_flat, wav_flat, nll, ptgt, hit):
        ptr = lambda t: t.data_ptr() if t is not None else None
        return (dict(codes=codes_flat.data_ptr(), n_codes=codes_flat.numel(), wavs=wav_flat.data_ptr(), n_wav=wav_flat.numel()),
                dict(dst_nll=nll.data_ptr(), n_dst=nll.numel(), dst_ptgt=ptr(ptgt), dst_hit=ptr(hit)))

    def score_batch_plan(self, codes_flat: torch.Tensor, wav_flat: torch.Tensor, table: torch.Tensor, table_host: torch.Tensor,
                         first_row: int, nll: torch.Tensor, ptgt: Optional[torch.Tensor] = None,
                         hit: Optional[torch.Tensor] = None) -> Plan:
        """One batch of a whole-utterance scoring as a plan of its own (for a caller's captured graph): [wav.tile] + the ops
        of score_plan() (the same records) + [nll.stitch] over the rows [first_row, first_row + B) of `table` (uint8 device
        bytes of aew_score_row_t records; table_host: the same bytes in pinned host memory, read at capture).  in_jitter is
        set to the identity and the decoder's weight layouts are packed here, once (after a change of the weights the
        caller runs decoder_pack_plan() again); the caller zeroes codes_bad / score_bad and keeps the tensors alive.  A
        deferred EMA accumulation is applied here, once, as evaluate() does at its head."""
        self.scoring_ops()
        self._score_check("score_batch_plan()", codes_flat, wav_flat, nll, ptgt, hit)
        self.finish_ema()                                            # (a deferred EMA accumulation first, as evaluate())
        self.in_jitter.copy_(torch.arange(self.geom.embed_len, device=self.device).expand(self.B, -1))
        self.decoder_pack_plan().run(self._stream())
        return self._tile_batch_plan("score.batch", self.score_tile, self.score_plan(), self.score_stitch,
                                     self._score_fields(codes_flat, wav_flat, nll, ptgt, hit), table, table_host, first_row,
                                     join=True)

    def score_tiles(self, codes_flat: torch.Tensor, wav_flat: torch.Tensor, table, nll: torch.Tensor,
                    ptgt: Optional[torch.Tensor] = None, hit: Optional[torch.Tensor] = None, *, offsets, acc: torch.Tensor,
                    out: torch.Tensor):
        """The teacher-forced likelihood of whole utterances through the fixed-geometry decoder: `codes_flat` int64 and
        `wav_flat` float32 (float-encoded mu-law values), the flat ragged buffers; `table` a numpy array of
        aew_score_row_t records (_lib.SCORE_ROW_DTYPE), a multiple of B rows (codes.ScoreTilePlan.table); `nll` - and
        `ptgt` float32, `hit` uint8 - the flat per-utterance outputs, utterance u owning [offsets[u], offsets[u + 1])
        (`offsets`: U + 1 host integers); `acc` float64 (U, 4) and `out` float32 (U, 4), what AEW_OP_SCORE_REDUCE writes.
        The table and the offsets go to the device once (one pinned buffer, non-blocking); per batch of B rows one
        AEW_OP_WAV_TILE fills in_wav / ind / in_voice, score_plan() runs with in_jitter the identity, and one
        AEW_OP_NLL_STITCH moves the outputs each window owns (_run_tiles); then one AEW_OP_SCORE_REDUCE.  Codes outside
        [0, K) become code 0 and count in `codes_bad[0]`, samples outside [0, n_quant) become the zero-amplitude code and
        count in `score_bad[0]` (both zeroed here; reading them synchronises).  Writes what codes_to_conditioning() writes,
        the decoder's activations and logits (act_epoch), the packed layouts of the decoder's weights
        (decoder_pack_plan(), once per call) and nothing else of the engine: none of emb, the EMA accumulators and
        statistics, ind_hist, loss_buf, met_buf, diag, eval_acc / eval_hist, the parameters, gradients, moments or the
        average.  A deferred EMA accumulation (forward() with an asynchronous statistics collective and no backward since)
        is applied first, as evaluate() does: the codebook read is the one behind that update.  No host synchronisation
        otherwise."""
        _, _, sr = self.scoring_ops()
        n = self._tile_rows("score_tiles()", table, L.ScoreRow, "aew_score_row_t")
        self._score_check("score_tiles()", codes_flat, wav_flat, nll, ptgt, hit)
        off = np.ascontiguousarray(np.asarray(offsets, np.int64).reshape(-1))
        U = len(off) - 1
        if U < 0 or acc.dtype != torch.float64 or tuple(acc.shape) != (U, 4) or not acc.is_contiguous() or \
                out.dtype != torch.float32 or tuple(out.shape) != (U, 4) or not out.is_contiguous():
            raise L.AewError(f"score_tiles(): offsets (U + 1,), acc float64 (U, 4) and out float32 (U, 4) expected")
        if U and (off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != nll.numel()):
            raise L.AewError("score_tiles(): offsets must ascend from 0 to len(nll)")
        self.codes_bad.zero_()
        self.score_bad.zero_()
        if U == 0 or nll.numel() == 0:                                    # nothing to score anywhere: empty rows, zero summaries
            acc.zero_()
            out.zero_()
            return
        self._chain_watch("check")
        self.finish_ema()
        self.in_jitter.copy_(torch.arange(self.geom.embed_len, device=self.device).expand(self.B, -1))
        if n:
            self.act_epoch += 1
            self.decoder_pack_plan().run(self._stream())
        tile_f, stitch_f = self._score_fields(codes_flat, wav_flat, nll, ptgt, hit)
        # (a table is a multiple of 64 bytes long: the offsets behind it stay aligned)
        dev, host = self._run_tiles(self.score_tile, self.score_plan(), self.score_stitch, (tile_f, stitch_f), table, (off,))
        try:
            sr.offsets, sr.offsets_host, sr.U = dev.data_ptr() + table.nbytes, host.data_ptr() + table.nbytes, U
            sr.nll, sr.n_src, sr.ptgt, sr.hit = stitch_f["dst_nll"], stitch_f["n_dst"], stitch_f["dst_ptgt"], stitch_f["dst_hit"]
            sr.acc, sr.out = acc.data_ptr(), out.data_ptr()
            self.score_reduce.run(self._stream())
            if n:
                self._chain_watch("fwd")
        finally:
            sr.offsets = sr.offsets_host = sr.nll = sr.ptgt = sr.hit = sr.acc = sr.out = None     # (as _run_tiles leaves its two)

    def conditioning(self):
        """Encoder / bottleneck and the conditioning half of the decoder forward only (jitter gather, lc_conv,
        upsampler, speaker bias): what the autoregressive sampler needs (wavenet.py:379-391).  No EMA statistics
        or update, no index histogram update (vq.stats is skipped), no loss.
        Returns (cond bf16 [B][T][Cp], gated bias fp32 [B][NL][2*Dp])."""
        self._cond_plans()
        self._run(self._cond_plan_a, False)
        self._run(self._cond_plan, False)
        return self._cond_out()

    # ---- chained launches: a hand-off wait that gave up must not pass silently --------------------------------------
    def _chain_flags(self):
        """[(label, 1-element int32 view of the launch's timeout flag)] over the engine's chained launches."""
        if self._chain_flag_views is None:
            v = []
            for pl in (self.fwd_b, self.bwd):
                for lab, (stages, cd) in getattr(pl, "nt_chains", {}).items():
                    n = sum(s.n_mt * s.g.batch for s in stages)
                    v.append((lab, cd[n:n + 1]))
            self._chain_flag_views = v
        return self._chain_flag_views

    CHAIN_WATCH_SLOTS = 4

    def _chain_watch(self, after: str):
        """The bounded spin of a chained launch (csrc/aew_chain.hip) ends a wait whose producer never arrives by setting a
        flag and letting the tile run on - with operands that may be incomplete.  Two things keep such a step from
        training on:
        * on the DEVICE the wait also raises the engine's sticky word (`chain_guard`, aew_nt_chain_t.sticky), which no plan
          clears and which the Adam and EMA / codebook ops read as their guard: from the poisoned step on they are no-ops,
          however far the host has run ahead;
        * on the HOST the sticky word is copied to pinned memory behind every plan that holds chained launches (`after` =
          "fwd" | "bwd"; asynchronous) into a ring of CHAIN_WATCH_SLOTS slots; "check" (the head of every forward) looks at
          every copy that has landed and raises.  A slot is reused only after its copy has been looked at - when the host is
          a full ring ahead it waits for the oldest copy (by then several plans old) - so no timeout is ever overwritten
          unseen, and one is reported at most CHAIN_WATCH_SLOTS plans late.  `chain_guard_check()` is the synchronous form
          for any point where the caller synchronises anyway."""
        if not self._chain_flags() or self.device.type != "cuda":
            return
        st = self._chain_host
        if st is None:
            n = self.CHAIN_WATCH_SLOTS
            st = self._chain_host = {"buf": torch.zeros(n, dtype=torch.int32).pin_memory(),
                                     "ev": [torch.cuda.Event() for _ in range(n)], "pending": []}
        if after == "check":
            self._chain_poll(False)
            return
        if len(st["pending"]) >= self.CHAIN_WATCH_SLOTS:
            self._chain_poll(True)
        used = set(st["pending"])
        slot = next(i for i in range(self.CHAIN_WATCH_SLOTS) if i not in used)
        st["buf"][slot:slot + 1].copy_(self.chain_guard[:1], non_blocking=True)
        st["ev"][slot].record()
        st["pending"].append(slot)

    def _chain_poll(self, wait_oldest: bool):
        st = self._chain_host
        while st["pending"]:
            slot = st["pending"][0]
            if not st["ev"][slot].query():
                if not wait_oldest:
                    return
                st["ev"][slot].synchronize()
            wait_oldest = False
            st["pending"].pop(0)
            if int(st["buf"][slot]) != 0:
                self._chain_raise(int(st["buf"][slot]))

    def _chain_raise(self, stage: int):
        torch.cuda.synchronize(self.device)
        bad = [lab for lab, f in self._chain_flags() if int(f.item()) != 0]      # (the per-launch flags of the LAST run)
        raise L.AewError(f"chained launch: a tile's wait for its producers gave up (aew_nt_chain_t spin limit; sticky word = "
                         f"stage {stage - 1} + 1; flagged in the last run: {bad}).  The optimizer and EMA updates have been "
                         "no-ops since that step (device-side guard); parameters are those of the step before.  "
                         "engine.clear_chain_guard() re-arms; AEW_NT_CHAIN=0 runs one launch per GEMM")

    def chain_guard_check(self):
        """Synchronous check of the sticky timeout word (for callers that synchronise anyway): raises like forward() would."""
        if self.device.type == "cuda":
            v = int(self.chain_guard[0].item())
            if v:
                self._chain_raise(v)

    def clear_chain_guard(self):
        """Re-arm after a reported timeout: clears the sticky word and forgets the copies in flight."""
        self.chain_guard.zero_()
        if self._chain_host is not None:
            torch.cuda.synchronize(self.device)
            self._chain_host["pending"].clear()
            self._chain_host["buf"].zero_()

    def _accum_run(self, acc: torch.Tensor, g: torch.Tensor, n: int, mode: int):
        """One launch of the accumulate op: fold g[0:n] into acc[0:n] (FIRST / ADD) or acc into g (LAST)."""
        if mode not in (L.ACCUM_FIRST, L.ACCUM_ADD, L.ACCUM_LAST):
            raise ValueError(f"Invalid accumulation mode: {mode!r} (0 FIRST, 1 ADD, 2 LAST)")
        if not self.accum.ops:
            self.accum.add(L.OP_ACCUM, L.Accum(), "accumulate", TAG_ADAM)
        a = self.accum.array()[0].u.accum
        a.acc, a.g, a.n, a.mode = acc.data_ptr(), g.data_ptr(), int(n), int(mode)
        self.accum.run(self._stream())

    def accum_grads(self, mode: int, lo: int = 0, hi: Optional[int] = None):
        """Gradient accumulation, one launch (AEW_OP_ACCUM) over the element range [lo, hi) (multiples of 4, like
        adam_step) of the flat gradient buffer and the running sum `acc_grads`: FIRST acc = g, ADD acc = acc + g, LAST
        g = acc + g (acc is left alone) - one fp32 addition per element, so a group's sum is ((g1 + g2) + g3) + ... in
        that order.  A data-parallel caller folds a region in as soon as it is final.  No host synchronisation."""
        hi = self.ps.numel if hi is None else hi
        assert lo % 4 == 0 and (hi % 4 == 0 or hi == self.ps.numel) and 0 <= lo <= hi <= self.ps.numel
        if self.acc_grads is None:
            self.acc_grads = self.ws.alloc("accum.grads", self.ps.numel, torch.float32)
        self._accum_run(self.acc_grads[lo:], self.ps.grads[lo:], hi - lo, mode)

    def accum_stats(self, mode: int):
        """The same fold over the EMA statistics of the batch (z_sum | n_sum; vqvae-ema only): after LAST they hold the
        sums over the group - n_sum exactly, its terms are integer counts."""
        if self.ema_plan is None:
            raise L.AewError(f"accum_stats() needs the vqvae-ema bottleneck (this engine: {self.bn_type})")
        n = self.zn_sum.numel()
        if self.acc_stats is None:
            self.acc_stats = self.ws.alloc("accum.stats", n, torch.float32)
        self._accum_run(self.acc_stats, self.zn_sum, n, mode)

    def forward(self, ema_allreduce=None, timing=False, before_decoder=None, accum: Optional[int] = None):
        """timing=True forces eager launches (the per-op event timing needs them).
        accum: None, or the fold (0 FIRST, 1 ADD, 2 LAST) of this micro-batch in a group of accumulated ones.  FIRST /
        ADD: the batch's EMA statistics go into the group's sums (accum_stats) and NO EMA is applied (fwd_b_noema), no
        statistics collective is issued.  LAST: z_sum / n_sum become the group's sums and the forward goes on as without
        accumulation - the cross-rank sum, then the EMA, once for the group.  Engines without EMA statistics: ignored.
        before_decoder(): called between the two forward plans - the first point at which a decoder parameter is read
        (pack_dec_late); a data-parallel caller waits there for the all-gather of the decoder's parameter shards.
        ema_allreduce(z_sum, n_sum): cross-rank sum of the EMA statistics.  If it returns a work handle
        (async collective) the EMA accumulation is deferred to finish_ema(), called by backward() - or by the next
        forward() if no backward came in between (forward-only use: the accumulation must not be lost)."""
        self._chain_watch("check")
        self.finish_ema(timing)
        self._run(self.fwd_a, timing)
        self.lin_live = True
        if before_decoder is not None:
            before_decoder()
        if accum is not None and self.ema_plan is not None:
            self.accum_stats(accum)
            if accum != L.ACCUM_LAST:                          # inside a group: no collective, no EMA
                self._run(self.fwd_b_noema, timing)
                if not timing:
                    self._chain_watch("fwd")
                return self.loss_buf[0]
        if ema_allreduce is not None and self.ema_plan is not None:
            work = ema_allreduce(self.z_sum, self.n_sum)
            if work is not None:
                self._ema_work = work
                self._run(self.fwd_b_noema, timing)
                if not timing:
                    self._chain_watch("fwd")
                return self.loss_buf[0]
        self._run(self.fwd_b, timing)
        if not timing:
            self._chain_watch("fwd")
        return self.loss_buf[0]

    def evaluate(self):
        """The loss of the batch in the inputs WITHOUT a training step: the forward plans minus EVAL_DROP, the loss into
        `eval_loss` and the batch folded into the running record (eval_acc / eval_hist, one launch).  Writes none of emb,
        ema_numer, ema_denom, ind_hist, z_sum, n_sum, n_sum_diag, loss_buf, met_buf, diag, diag_pk, gstat, the
        parameters, gradients, Adam moments or average, step_count, weights_version.  It DOES overwrite the activations,
        code indices and logits: a backward of an earlier forward() is no longer possible (act_epoch).  A deferred EMA
        accumulation is applied first, as forward() does; no host synchronisation.  Returns the 0-d device loss."""
        ea, eb, _ = self.eval_plans()
        self._chain_watch("check")
        self.finish_ema()
        self.act_epoch += 1
        self._run(ea, False)
        self._run(eb, False)
        if self.eval_grouping:                     # the batch once more, per window, into the record of in_group's ids
            self._run(self.eval_g, False)
        self._chain_watch("fwd")
        return self.eval_loss[0]

    def eval_reset(self):
        """Start a new record (zeroes eval_acc / eval_hist on the device)."""
        self.eval_plans()
        self.eval_acc.zero_()
        self.eval_hist.zero_()

    def eval_finish(self) -> torch.Tensor:
        """Finalize launch: the record as means -> eval_out (float [16] device view, _lib.EVAL_OUT_NAMES); the record itself
        is left as it is, so more batches may follow.  Reading the view is the caller's synchronisation."""
        self._run(self.eval_plans()[2], False)
        return self.eval_out

    def eval_group_reset(self, G: Optional[int] = None):
        """Start a new grouped record (zeroes eval_gacc / eval_ghist / eval_gtot / eval_win on the device) for G groups
        - default: as many as the record has - and switch grouping on: every evaluate() from here on also folds its
        batch by the ids in in_group."""
        if G is None and self.eval_gfin is None:
            raise L.AewError("eval_group_reset(): no grouped evaluation record yet; give the number of groups")
        self.eval_group_plans(self.eval_G if G is None else G)
        for t in (self.eval_gacc, self.eval_ghist, self.eval_gtot, self.eval_win):
            if t is not None:
                t.zero_()
        self.eval_grouping = True

    def eval_group_finish(self):
        """Finalize launch of the grouped record -> (eval_gout float [G][12], eval_tout float [16]) device views
        (_lib.EVAL_GOUT_NAMES / EVAL_TOUT_NAMES); the record is left as it is.  Reading a view is the caller's
        synchronisation."""
        if self.eval_gfin is None:
            raise L.AewError("eval_group_finish(): no grouped evaluation record (eval_group_reset() starts one)")
        self._run(self.eval_gfin, False)
        return self.eval_gout, self.eval_tout

    def finish_ema(self, timing=False):
        """Deferred vq.ema (see forward): wait for the statistics' all-reduce, then accumulate."""
        if self._ema_work is not None:
            self._ema_work.wait()
            self._ema_work = None
            self._run(self.ema_plan, timing)

    def set_upstream_grad(self, g):
        """d(L)/d(loss) for the next backward(): a python float or a 0-d tensor (copied device-side, no sync)."""
        if torch.is_tensor(g):
            self.gmul[:1].copy_(g.detach().reshape(1).to(self.gmul.dtype), non_blocking=True)
        else:
            self.gmul[:1].fill_(float(g))

    def backward(self, timing=False, after_decoder=None, after_decoder_hi=None, refresh_codebook: bool = True):
        """refresh_codebook=False: the backward of a micro-batch inside a group of accumulated ones - no EMA ran in its
        forward, so the codebook that follows the EMA statistics is not refreshed either (update_codebook_every_step).
        after_decoder: optional callback invoked between the decoder part of the backward (all
        decoder gradients final in ps.grads[dec_grad_offset:]) and the bottleneck / encoder part.
        after_decoder_hi: optional callback invoked as soon as ps.grads[dec_hi_offset:] is final (engines built with two
        grouped weight-gradient launches only: dec_hi_offset is not None)."""
        if after_decoder is None or not self.bwd_b.ops:
            self._run(self.bwd, timing)
            if after_decoder_hi is not None and self.dec_hi_offset is not None:
                after_decoder_hi()
            if after_decoder is not None:
                after_decoder()
        else:
            if after_decoder_hi is not None and self.bwd_a1 is not None:
                self._run(self.bwd_a1, timing)
                after_decoder_hi()
                self._run(self.bwd_a2, timing)
            else:
                self._run(self.bwd_a, timing)
            after_decoder()
            self._run(self.bwd_b, timing)
        if not timing and self.nt_chain_bwd_used >= 2:
            self._chain_watch("bwd")
        self.finish_ema(timing)
        if self.update_codebook_every_step and self.ema_plan is not None and refresh_codebook:     # (the codebook that follows the EMA statistics)
            self._run(self.cb, timing)

    def update_codebook(self):
        self.finish_ema()
        self.cb.run(self._stream())

    def _restart_op(self) -> L.VqRestart:
        """The restart op, allocated with its two output buffers (and the `restart` plan completed) at its first use."""
        if self.ema_plan is None:
            raise L.AewError(f"restarting codes needs the vqvae-ema bottleneck (this engine: {self.bn_type}): only its "
                             "codebook carries a usage statistic")
        if self.restart_buf is None:
            self.restart_buf, self.restart_pairs_buf, rs = self.bn.restart_op()
            self.restart.add(L.OP_VQ_RESTART, rs, "vq.restart", TAG_VQ)
        return self.restart.array()[0].u.vqr

    def restart_codes(self, min_usage: float, call: int, max_codes: int = 64, denom_init: float = 1.0, seed: int = 0):
        """Re-seed dead codes on the device (AEW_OP_VQ_RESTART, one launch, no host synchronisation): every code k with
        !(ema_denom[k] >= min_usage), ascending, at most min(Q, max_codes) of them, takes a distinct row of this step's
        encoder outputs (bn.lin) chosen by the counter-based hash of (seed, call): ema_numer[k] = ze * denom_init,
        emb[k] = ema_numer[k] / denom_init, ema_denom[k] = denom_init.  A pending EMA accumulation is applied first (it
        would overwrite the restart); a raised chain_guard makes the launch a no-op.  Counts: restart_out()."""
        if self.ema_plan is None:
            self._restart_op()                                          # raises: nothing is allocated for a refused call
        if not self.lin_live:
            raise L.AewError("restart_codes() before any forward on this engine: bn.lin holds no encoder output yet")
        if not 1 <= int(max_codes) <= L.VQ_RESTART_MAX:
            raise ValueError(f"Invalid max_codes: {max_codes} (1 .. {L.VQ_RESTART_MAX})")
        if not (math.isfinite(denom_init) and denom_init > 0.0):
            raise ValueError(f"Invalid denom_init: {denom_init} (finite, > 0)")
        if math.isnan(min_usage):
            raise ValueError("Invalid min_usage: nan")
        if call < 0 or seed < 0:
            raise ValueError(f"Invalid call / seed: {call} / {seed} (unsigned 64-bit counters)")
        self.finish_ema()
        rs = self._restart_op()
        rs.min_usage, rs.denom_init, rs.max_codes = float(min_usage), float(denom_init), int(max_codes)
        rs.seed, rs.call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
        self.restart.run(self._stream())

    def restart_out(self) -> torch.Tensor:
        """int32 [4] device view: dead codes found and codes restarted by the last restart_codes(), codes restarted since
        the engine was built, 0.  Reading it is the caller's synchronisation."""
        self._restart_op()
        return self.restart_buf

    def restart_pairs(self) -> torch.Tensor:
        """int32 [AEW_VQ_RESTART_MAX][2] device view: (code, row of bn.lin) of the last launch's restarts in order, (-1, -1)
        behind them up to its max_codes."""
        self._restart_op()
        return self.restart_pairs_buf

    def grad_norm_step(self, ranges, max_grad_norm: float, grad_scale: float = 1.0, finalize: bool = True,
                       add_partial: bool = False):
        """One launch of the gradient-norm op over element ranges [(lo, hi), ...] of the flat gradient buffer (lo a
        multiple of 4, hi >= lo; empty ranges allowed, at most 8).  finalize=True: the total goes to clip_sumsq[0] and
        norm / coefficient / flag / skip count to clip_out (what adam_step(max_grad_norm=...) reads).  finalize=False:
        the sum goes to clip_sumsq[1] only - a sharded caller all-reduces that word and passes add_partial=True to the
        finalizing launch, which adds it in.  No host synchronisation.
        More than 8 ranges (the trainable tensors of a step with frozen ones, trainable_ranges): a chain of launches in
        stream order, each over up to 8 ranges - all but the last leave their running sum in clip_sumsq[1]
        (finalize = 0), the next adds it in (add_in)."""
        if not (max_grad_norm > 0):
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        K = L.GRAD_NORM_MAX_RANGES
        if len(ranges) > K:
            for i in range(0, len(ranges), K):
                last = i + K >= len(ranges)
                self.grad_norm_step(ranges[i:i + K], max_grad_norm, grad_scale, finalize=finalize and last,
                                    add_partial=add_partial or i > 0)
            return
        g = self.clip.array()[0].u.gnorm
        if not 1 <= len(ranges):
            raise ValueError("at least one range")
        for i in range(L.GRAD_NORM_MAX_RANGES):
            lo, hi = ranges[i] if i < len(ranges) else (0, 0)
            assert lo % 4 == 0 and 0 <= lo <= hi <= self.ps.numel
            g.x[i], g.n[i] = self.ps.grads.data_ptr() + 4 * lo, hi - lo
        g.n_ranges, g.finalize = len(ranges), int(finalize)
        g.add_in = self.clip_sumsq.data_ptr() + 8 if add_partial else None
        g.sumsq = self.clip_sumsq.data_ptr() + (0 if finalize else 8)
        g.max_norm, g.grad_scale, g.eps = float(max_grad_norm), float(grad_scale), 1e-6
        self.clip.run(self._stream())

    def grad_norm(self) -> torch.Tensor:
        """Device view [4] of the last clipped step: total gradient norm (of grad_scale * g), clip coefficient, non-finite
        flag, steps skipped so far.  Reading it is the caller's synchronisation."""
        return self.clip_out[:4]

    def ratio_step(self, finalize: bool = True, add_partial: bool = False):
        """One launch of the update-ratio op over the chunk sums the tracked Adam calls of this step left.  finalize=True:
        per-tensor update norm, weight norm and ratio go to uw_out (what update_ratios() returns).  finalize=False: the
        per-tensor fp64 pairs go to uw_sums only - a sharded caller all-reduces those 2 P words and then passes
        finalize=True, add_partial=True, which takes the totals from uw_sums alone.  No host synchronisation."""
        if self._uw_zero:                                # no tracked Adam call since the step began: nothing was summed
            self.uw_part.zero_()
            self._uw_zero = False
        r = self.ratio.array()[0].u.ratio
        r.finalize = int(finalize)
        r.part = None if add_partial else self.uw_part.data_ptr()
        r.add_in = self.uw_sums.data_ptr() if add_partial else None
        self.ratio.run(self._stream())
        self._uw_stale = not finalize

    def update_ratios(self) -> torch.Tensor:
        """Device view [3][P] of the last tracked step, P tensors in ps.names() order: update norm ||p_old - p_new||,
        weight norm ||p_old||, their ratio (chassis.py:180-183).  A step made of range calls is reduced here, once, when
        its results are first asked for.  Reading the view is the caller's synchronisation."""
        if self._uw_stale:
            self.ratio_step()
        return self.uw_out[:3 * self.uw_n].view(3, self.uw_n)

    def adam_step(self, lr: float, grad_scale: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8,
                  lo: int = 0, hi: Optional[int] = None, count: bool = True, max_grad_norm: Optional[float] = None,
                  norm_done: bool = False, track: bool = False, avg_rate: Optional[float] = None, groups=None):
        """One Adam step over the flat buffer, or over its element range [lo, hi) (multiples of 4): a
        data-parallel caller updates the decoder tail while the encoder gradients are still being
        reduced (`count=False` on all but the first range of a step).
        max_grad_norm: clip the gradient to this global norm (torch.nn.utils.clip_grad_norm_): the first range of a step
        (count=True) runs the norm plan over the WHOLE buffer first - every gradient must be final by then - and every
        range multiplies the coefficient in; a step whose norm is inf / nan changes nothing on the device (step_count
        still advances, like a step the chain guard stopped).  norm_done=True: the caller has run grad_norm_step()
        itself (sharded data parallel).  None: the op reads no clip word - the step of an engine without clipping.
        track: the launch also sums (p_old - p_new)^2 and p_old^2 per chunk of the parameter tensors it covers
        (aew_uw_track_t); the first tracked call of a step clears the sums, a whole-buffer step reduces them to
        update_ratios() right away, range calls leave that to the accessor.  False: the op carries no record.
        avg_rate: the launch also moves the averaged weights (adam_avg, aew_adam_t.avg) of the elements it updates towards
        their new values, avg += avg_rate * (p_new - avg), avg_rate = 1 - decay of this step; the first averaged call of
        an engine without an average starts it from the parameters in front of that step.  A step the device skips leaves
        the average alone; avg_steps advances with count like step_count.  None: the op carries no average.
        groups: one (lr, weight_decay, frozen) per parameter tensor in ps.names() order (aew_adam_groups_t): every tensor
        is stepped with its own rate and decoupled decay, a frozen one is left alone, and the clip norm of the step covers
        the trainable tensors only (trainable_ranges).  `lr` is then not read.  None: the op carries no record - the
        launch of an engine without groups, grid and bits."""
        if self.averaged_in:
            raise L.AewError("adam_step() while the averaged weights are swapped in: the step would update the average "
                             "in the parameters' place (leave FusedAdam.averaged_weights() / call swap_averaged() first)")
        if avg_rate is not None and not 0.0 <= float(avg_rate) <= 1.0:
            raise ValueError(f"Invalid avg_rate: {avg_rate} (1 - decay, within [0, 1])")
        hi = self.ps.numel if hi is None else hi
        assert lo % 4 == 0 and (hi % 4 == 0 or hi == self.ps.numel) and 0 <= lo < hi <= self.ps.numel
        if groups is not None:
            self._groups_table(groups)                   # (refuses a malformed list; uploads the records when they changed)
        # every argument is checked by here: a refused call leaves the counters and the average as they were
        if avg_rate is not None:
            if not self.avg_live:
                n = self.ps.numel
                self._avg_buffer()[:n].copy_(self.ps.params[:n])
                self.avg_live = True
            if count:
                self.avg_steps += 1
        if count:
            self.step_count += 1
            self._uw_zero = True
        self.weights_version += 1
        if max_grad_norm is not None and count and not norm_done:
            self.grad_norm_step(self.trainable_ranges(groups), max_grad_norm, grad_scale)
        # (with groups: the op of its own that carries the descriptor and the group record - the `opt` plan is untouched)
        plan = self.opt if groups is None else self.opt_groups
        a = plan.array()[0].u.adam if groups is None else plan.array()[0].u.adamg.adam
        a.p, a.g = self.ps.params.data_ptr() + 4 * lo, self.ps.grads.data_ptr() + 4 * lo
        a.m, a.v = self.adam_m.data_ptr() + 4 * lo, self.adam_v.data_ptr() + 4 * lo
        a.n = hi - lo
        a.lr, a.beta1, a.beta2, a.eps = lr, betas[0], betas[1], eps
        a.bc1 = 1.0 - betas[0] ** self.step_count
        a.bc2 = 1.0 - betas[1] ** self.step_count
        a.grad_scale = grad_scale
        a.clip = self.clip_out.data_ptr() + 4 if max_grad_norm is not None else None
        a.avg, a.avg_rate = (self._avg_buffer().data_ptr() + 4 * lo, float(avg_rate)) if avg_rate is not None else (None, 0.0)
        a.track = None
        if track:
            self.uw_track.base, self.uw_track.zero = lo, int(self._uw_zero)
            a.track = C.addressof(self.uw_track)
            self._uw_zero = False
        if groups is not None:
            self.adam_groups.base = lo
        plan.run(self._stream())
        if track:
            if lo == 0 and hi == self.ps.numel:
                self.ratio_step()
            else:
                self._uw_stale = True

    # ---- parameter groups: the device table of tensor records and the element ranges of the trainable tensors
    GROUPS_RING_SLOTS = 4

    def _groups_table(self, groups):
        """The device table of P aew_adam_tensor_t records for `groups` = [(lr, weight_decay, frozen)] in ps.names()
        order.  Allocated at its first use; uploaded only when a record differs from what the table holds, in stream
        order and without a host-device synchronisation: the bytes go through a ring of GROUPS_RING_SLOTS pinned slots,
        and a slot is rewritten only when the copy that last read it is complete (in practice long ago: four changes of
        the table back)."""
        raw = L.adam_tensor_records(groups, self.uw_n)
        P = self.uw_n
        if self.adam_groups_tbl is None:
            self.adam_groups_tbl = self.ws.alloc("adam.groups", 4 * P, torch.int32)
            self.adam_groups.tensors = self.adam_groups_tbl.data_ptr()
            ag = L.AdamGrouped()                         # the op: `opt`'s descriptor (re-addressed per call) + the record
            ag.adam = self.opt.array()[0].u.adam          # (a copy: the guard word and the buffers)
            ag.groups = C.addressof(self.adam_groups)
            self.opt_groups.add(L.OP_ADAM_GROUPS, ag, "adam (groups)", TAG_ADAM)
        if raw == self._groups_sent:
            return
        src = torch.frombuffer(bytearray(raw), dtype=torch.int32)
        if self.device.type == "cuda":
            ring = self._groups_ring
            if ring is None:
                n = self.GROUPS_RING_SLOTS
                ring = self._groups_ring = {"buf": torch.zeros(n, 4 * P, dtype=torch.int32).pin_memory(),
                                            "ev": [torch.cuda.Event() for _ in range(n)], "next": 0}
            slot = ring["next"]
            ring["next"] = (slot + 1) % self.GROUPS_RING_SLOTS
            ring["ev"][slot].synchronize()               # (returns at once for an event that was never recorded)
            ring["buf"][slot].copy_(src)
            self.adam_groups_tbl[:4 * P].copy_(ring["buf"][slot], non_blocking=True)
            ring["ev"][slot].record()
        else:
            self.adam_groups_tbl[:4 * P].copy_(src)
        self._groups_sent = raw

    def trainable_ranges(self, groups, within=None):
        """Element ranges [(lo, hi)] of the flat buffer, ascending and merged, that the tensors `groups` does not freeze
        cover (their pad elements included; None: the whole buffer) - what the clip norm of a grouped step is taken over.
        within: [(a, b)] - the ranges are cut to these (a sharded caller's shards and remainders), in their order.  Never
        empty: (0, 0) stands for "nothing"."""
        if groups is None:
            merged = [(0, self.ps.numel)]
        else:
            assert len(groups) == self.uw_n
            merged = []
            for (lo, hi), g in zip(self._tensor_span, groups):
                if g[2] or hi == lo:
                    continue
                if merged and merged[-1][1] == lo:
                    merged[-1] = (merged[-1][0], hi)
                else:
                    merged.append((lo, hi))
        if within is not None:
            merged = [(max(lo, a), min(hi, b)) for a, b in within for lo, hi in merged if max(lo, a) < min(hi, b)]
        return merged or [(0, 0)]

    def _avg_buffer(self) -> torch.Tensor:
        """adam_avg, allocated (and the swap plan completed) at its first use; avg_live becomes True only behind a call."""
        if self.adam_avg is None:
            self.adam_avg = self.ws.alloc("adam.avg", self.ps.numel, torch.float32)
            sw = L.Swap()
            sw.a, sw.b, sw.n = self.ps.params.data_ptr(), self.adam_avg.data_ptr(), self.ps.numel
            self.swap.add(L.OP_SWAP, sw, "swap averaged weights", TAG_ADAM)
        return self.adam_avg

    # ---- the optimizer state as one record: nothing outside this class writes step_count, avg_steps, avg_live,
    # averaged_in or (but for dp.gather_moments, in place, through opt_buffers) the three flat buffers
    def opt_buffers(self) -> tuple:
        """The flat state buffers that hold values: adam_m, adam_v and, once there is an average, adam_avg."""
        return (self.adam_m, self.adam_v) + ((self.adam_avg,) if self.avg_live else ())

    def opt_state(self, clone: bool) -> OptState:
        """The state as views of the engine's buffers, or as clones that outlive it."""
        n = self.ps.numel
        m, v, *avg = [b[:n].detach().clone() if clone else b[:n] for b in self.opt_buffers()]
        return OptState(self.step_count, m, v, self.avg_steps, avg[0] if avg else None, self.averaged_in)

    def load_opt_state(self, st: OptState):
        """Take a record in (tensors from any device).  One without an average leaves the engine without one: the
        average then starts again from the parameters at the next averaged step."""
        n = self.ps.numel
        self.adam_m[:n].copy_(st.m)
        self.adam_v[:n].copy_(st.v)
        self.step_count = int(st.step)
        if st.avg is not None:
            self._avg_buffer()[:n].copy_(st.avg)
            self.avg_steps, self.avg_live, self.averaged_in = int(st.avg_steps), True, bool(st.averaged_in)
        else:
            self.avg_steps, self.avg_live, self.averaged_in = 0, False, False

    def swap_averaged(self):
        """Exchange the parameters with their average on the device (AEW_OP_SWAP, one pass, no third buffer): after an odd
        number of calls forward / sampling / state_dict see the averaged weights and adam_avg holds the raw ones
        (`averaged_in`); adam_step() refuses to run until they are swapped back.  Everything that keeps a packed copy of
        the weights re-packs (weights_version)."""
        if not self.avg_live:
            raise L.AewError("no averaged weights yet: no optimizer step with an average has run on this engine")
        self.swap.run(self._stream())
        self.weights_version += 1
        self.averaged_in = not self.averaged_in

    # --------------------------------------------------------------------------------------
    # views for the module surface / tests
    # --------------------------------------------------------------------------------------
    def logits(self) -> torch.Tensor:
        """(B, w, Q) fp32 channels-last view."""
        return self.dec.logits.tensor()[:, :, :self.hps.n_quant]

    def init_ema_from_emb(self):
        """vqema_bn.py:117-118."""
        comp = 1.0 - self.hps.bn_vq_ema_gamma
        self.ema_numer.copy_(self.emb * comp)
        self.ema_denom.fill_(comp)

    def flops_per_step(self) -> Dict[str, float]:
        """Algorithmic FLOPs of one training step by the formula of SURVEY Appendix B /
        BASELINE.md §4 (decoder stack + post network; x3 for fwd + dgrad + wgrad)."""
        h, g = self.hps, self.geom
        R, D, S, P, Q = h.n_res, h.n_dil, h.n_skp, h.n_post, h.n_quant
        C = h.n_lc_out + h.n_global_embed
        nl = len(g.layers)
        mac = 0
        for i, lg in enumerate(g.layers):
            mac += lg.out_len * (2 * 2 * R * D + 2 * C * D + (D * R if i < nl - 1 else 0))
        mac += nl * g.n_win * D * S + g.n_win * (S * P + P * Q)
        fwd = 2.0 * mac * self.B
        return {"fwd": fwd, "step": 3.0 * fwd}
