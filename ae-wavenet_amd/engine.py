"""Launch plans for the WaveNet-autoencoder training step.

Builds, once per (model, batch, window), the forward and backward plans that
`aew_run_plan` executes: weight packing, encoder (fp32 exact chain), bottleneck, the
conditioning path, the gated dilated stack, the post network, the loss, and the complete
hand-written backward including weight-gradient GEMMs and gradient unpacking.

Reference arithmetic restated by these plans (citations into the reference checkout):
  encoder            wave_encoder.py:34-50, 53-103
  bottlenecks        vqema_bn.py:125-222, vq_bn.py:28-61, vae_bn.py:26-62, ae_bn.py:11-16
  decoder            wavenet.py:91-111 (gated layer), :127-140 (conditioning), :142-165
                     (upsampling), :323-364 (forward_train)
  losses             wavenet.py:541-552, vqema_bn.py:231-266, vq_bn.py:72-115,
                     vae_bn.py:76-125, ae_bn.py:29-46
  wiring             autoencoder_model.py:206-259, mfcc_inverter.py:89-108
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib as L
from . import geometry as G
from .plan import (CopyTableBuilder, ESIZE, Mat, Plan, TnGroupBuilder, Workspace, make_nt, make_tn, null_view, ru)

BF, F3 = L.BF16, L.F32

# timing tags (reported by aew_timing_read; bench.py groups kernel time by these)
TAG_G1, TAG_G2, TAG_DZ, TAG_DX, TAG_WG_FG, TAG_WG_RS, TAG_DCOND, TAG_POST, TAG_UPS, TAG_ENC, \
    TAG_VQ, TAG_LOSS, TAG_PACK, TAG_MISC, TAG_ADAM = range(1, 16)


# ------------------------------------------------------------------------------------------
# parameters
# ------------------------------------------------------------------------------------------
def decoder_param_specs(hps, n_lc_in: int, pre: str) -> List[Tuple[str, Tuple[int, ...]]]:
    """Names / shapes / registration order of the reference WaveNet module
    (wavenet.py:184-259)."""
    R, D, S, P, Q = hps.n_res, hps.n_dil, hps.n_skp, hps.n_post, hps.n_quant
    Cc = hps.n_lc_out + hps.n_global_embed
    sp: List[Tuple[str, Tuple[int, ...]]] = [(pre + "lc_conv.weight", (hps.n_lc_out, n_lc_in, 3))]
    if hps.bias:
        sp.append((pre + "lc_conv.bias", (hps.n_lc_out,)))
    for i, f in enumerate(hps.lc_upsample_filt_sizes):
        sp.append((pre + f"lc_upsample.{i}.tconv.weight", (hps.n_lc_out, hps.n_lc_out, f)))
        sp.append((pre + f"lc_upsample.{i}.tconv.bias", (hps.n_lc_out,)))
    sp.append((pre + "cond.speaker_embedding.weight", (hps.n_global_embed, hps.n_speakers)))
    sp.append((pre + "cond.speaker_embedding.bias", (hps.n_global_embed,)))
    sp.append((pre + "base_layer.weight", (R, Q, 1)))
    if hps.bias:
        sp.append((pre + "base_layer.bias", (R,)))
    nl = hps.n_blocks * hps.n_block_layers
    for i in range(nl):
        p = pre + f"conv_layers.{i}."
        for nm in ("conv_signal", "conv_gate"):
            sp.append((p + nm + ".weight", (D, R, 2)))
            if hps.bias:
                sp.append((p + nm + ".bias", (D,)))
        sp.append((p + "proj_signal.weight", (D, Cc, 1)))
        sp.append((p + "proj_gate.weight", (D, Cc, 1)))
        sp.append((p + "dil_skp.weight", (S, D, 1)))
        if i != nl - 1:
            sp.append((p + "dil_res.weight", (R, D, 1)))
    for nm, shp in (("post1", (P, S, 1)), ("post2", (Q, P, 1))):
        sp.append((pre + nm + ".weight", shp))
        if hps.bias:
            sp.append((pre + nm + ".bias", (shp[0],)))
    return sp


def encoder_param_specs(n_in: int, n_out: int, pre: str = "encoder."):
    sp = []
    cin = n_in
    for i, f in enumerate(G.ENCODER_FILTERS):
        sp.append((pre + f"net.{i}.conv.weight", (n_out, cin, f)))
        sp.append((pre + f"net.{i}.conv.bias", (n_out,)))
        cin = n_out
    return sp


def bottleneck_param_specs(hps, pre: str = "bottleneck."):
    bn, E, d = hps.bn_type, hps.enc_n_out, hps.bn_n_out
    if bn == "vae":
        return [(pre + "linear.weight", (2 * d, E, 1))]
    if bn == "ae":
        return [(pre + "linear.weight", (d, E, 1)), (pre + "linear.bias", (d,))]
    if bn == "vqvae":
        # nn.Module registers direct Parameters before sub-module parameters (vq_bn.py:13,20)
        return [(pre + "emb", (hps.bn_vq_n_embed, d)), (pre + "linear.weight", (d, E, 1))]
    return [(pre + "linear.weight", (d, E, 1))]


class ParamStore:
    """All trainable parameters in one flat fp32 buffer (+ a same-shaped gradient buffer):
    one all-reduce, one fused Adam launch, and the pack/unpack tables address it by offset."""

    def __init__(self, ws: Workspace, specs: Sequence[Tuple[str, Tuple[int, ...]]]):
        self.ws = ws
        self.shape: Dict[str, Tuple[int, ...]] = {}
        self.off: Dict[str, int] = {}
        o = 0
        for n, shp in specs:
            self.shape[n], self.off[n] = tuple(shp), o
            numel = 1
            for s in shp:
                numel *= s
            o += ru(numel, 4)
        self.numel = o
        self.params = ws.alloc("params", o, torch.float32)
        self.grads = ws.alloc("grads", o, torch.float32)

    def names(self):
        return list(self.shape)

    def numel_of(self, n):
        k = 1
        for s in self.shape[n]:
            k *= s
        return k

    def view(self, n, grad=False) -> torch.Tensor:
        t = self.grads if grad else self.params
        return t[self.off[n]:self.off[n] + self.numel_of(n)].view(self.shape[n])

    def ptr(self, n, grad=False) -> int:
        t = self.grads if grad else self.params
        return t.data_ptr() + 4 * self.off[n]

    def has(self, n):
        return n in self.shape


# ------------------------------------------------------------------------------------------
# pack / unpack helpers
# ------------------------------------------------------------------------------------------
def _gate_groups(D: int):
    """Output channel co -> packed row (co//16)*32 + co%16 (+16 for gate).  Yields
    (co_start, n_groups, group_len) pieces covering [0, D)."""
    full = D // 16
    if full:
        yield 0, full, 16
    if D % 16:
        yield full * 16, 1, D % 16


class Piece(NamedTuple):
    """One rectangular piece of the index map between a parameter tensor and a packed matrix, stated once for both
    directions: p_* address the parameter (elements, relative to it), m_* the matrix.  A weight-gradient slab with the
    matrix's layout is unpacked by the pieces that pack the matrix."""
    pname: str
    p_off: int
    p_strides: Sequence[int]
    dims: Sequence[int]
    m_off: int
    m_strides: Sequence[int]

    def at(self, m_off: int, m_strides: Sequence[int]) -> "Piece":
        """The same parameter elements in another matrix layout (dgrad copies of a weight)."""
        return self._replace(m_off=m_off, m_strides=m_strides)


# where a weight gradient lands: `slabs` fp32 partial results `stride` elements apart, summed into the flat gradients by table `tbl`
WGrad = NamedTuple("WGrad", [("ptr", int), ("stride", int), ("slabs", int), ("tbl", CopyTableBuilder)])


def wgrad_slab(ws: Workspace, name: str, t: "L.GemmTN", slabs: int, tbl: CopyTableBuilder) -> WGrad:
    """Allocates the result of a TN descriptor (`slabs` partial sums of N_pad x K_total) and points the descriptor at it."""
    stride = t.N_pad * t.K_total
    ptr = ws.alloc(name, slabs * stride, torch.float32).data_ptr()
    t.out, t.out_batch_stride = ptr, stride
    return WGrad(ptr, stride, slabs, tbl)


class Packer:
    """Emits strided-copy records in both directions for the pieces of packed matrices:
    pack   params(fp32)        -> packed weights (bf16 / f32)
    unpack wgrad slabs (fp32)  -> flat grads (fp32), summing the slabs."""

    def __init__(self, ps: ParamStore, pack_tbl: CopyTableBuilder, unpack_tbl: CopyTableBuilder,
                 late_tbl: Optional[CopyTableBuilder] = None, first_tbl: Optional[CopyTableBuilder] = None):
        self.ps, self.pack_tbl, self.unpack_tbl = ps, pack_tbl, unpack_tbl
        self.late_tbl = late_tbl            # packs that only the backward reads (dgrad layouts): off the forward's start
        self.first_tbl = first_tbl          # packs the very first GEMM of the step needs (first=True): the only ones it waits for

    def pack(self, pc: Piece, w_mat: Mat, late: bool = False, first: bool = False):
        tbl = self.late_tbl if (late and self.late_tbl is not None) else self.pack_tbl
        if first and not late and self.first_tbl is not None:
            tbl = self.first_tbl
        tbl.add(self.ps.ptr(pc.pname) + 4 * pc.p_off, w_mat.ptr + pc.m_off * ESIZE[w_mat.dtype],
                pc.dims, pc.p_strides, pc.m_strides, F3, w_mat.dtype)

    def unpack(self, pieces: Sequence[Piece], g: WGrad):
        """The gradients of the pieces out of result g (the table is g's: the router's choice, or this packer's own)."""
        for pc in pieces:
            g.tbl.add(g.ptr + 4 * pc.m_off, self.ps.ptr(pc.pname, grad=True) + 4 * pc.p_off, pc.dims, pc.m_strides,
                      pc.p_strides, F3, F3, red_n=g.slabs, red_stride=g.stride)


# ------------------------------------------------------------------------------------------
# decoder
# ------------------------------------------------------------------------------------------
class DecoderPlan:
    """Conditioning path + gated stack + post network + NLL, forward and backward."""

    EARLY_LANE = 5            # side lane of the early halves below (the wgrads rotate over lanes 1..n_side_lanes)
    split_multiseg = False    # True: skip-sum / cond-gradient GEMMs as two halves, the early half on a side lane.
                              # Measured 8.31-8.34 vs 8.34-8.39 ms/step, but the bf16 partial sum costs accuracy (one
                              # gradient at 15.1 % of its max against the oracle, limit 15 %): off
    n_side_lanes = 4          # weight gradients / column sums rotate over this many side lanes (1..4): they are
                              # mutually independent, so they need no ordering among themselves.  Measured
                              # ms/step: 1 lane 8.44, 2: 8.54, 3: 8.59, 4: 8.19 (one lane per op kind: 8.93)
    # Ops that run on the full-N loader / consumer kernels (csrc/aew_fn.hip, impl 2; bit-identical results):
    #   "layer"  the gated pair of a layer as ONE fused op (gated GEMM -> z tile in LDS -> residual 1x1 + add)
    #   "G1"     gated GEMM alone on the full-N kernel (when "layer" is off or for the last layer)
    #   "dx" "dz" "skip" "dcond" "post"   the other large NT GEMMs of the stack
    # Default: the two long-K multi-segment GEMMs (K = 20 x 256: skip sum, cond gradient), where the loader / consumer
    # pipeline wins (0.170 vs 0.187 ms, 0.224 vs 0.248 ms).  The fused layer and the other ops are measured SLOWER than
    # the tiled kernels on this workload (fused layer 100-121 us vs 77-104 us for the pair; profiles/r02_notes.md:
    # with one block per CU nothing runs under the epilogue's 220 KB of stores per tile) and stay opt-in (AEW_FN_OPS).
    fn_ops = frozenset(("skip", "dcond"))
    wgrad_group = 64          # weight gradients of the gated stack (fg + res per layer), the skip weights and the post
                              # network as grouped launches (AEW_OP_GEMM_TN_GROUP) of this many layers: every output
                              # tile contracts over the whole time axis and batch in one block - one fp32 result per
                              # matrix instead of 8-90 split-K slabs that the unpack has to read back, and the ones-
                              # channel column gives the per-batch bias sums as running snapshots.  >= n_layers: ONE
                              # launch after the chain (768 tiles for the 20-layer stack = 3 blocks per CU); smaller
                              # groups run under the chain but were measured slower (a group of 8 layers is ~270 blocks
                              # of 0.9 ms each: one block per CU is bound by its own fill latency, and the chain's
                              # kernels lose the LDS those blocks hold: 8.63 / 9.68 ms per step with groups of 8 / 4
                              # against 7.68 with one launch and 7.75 with one split-K op per matrix).  0: one TN op per
                              # matrix (round 2's form)
    side_inputs_first = True  # forward: spk_bias / base_gather at the head of the plan's side lane (False: after the upsamplers)
    wgrad_tile = None         # output tile of the grouped wgrad launch: 128 (three 4-wave blocks per CU) | 256 (one 8-wave
                              # block per CU, half the operand bytes staged per FLOP) | None = by the size of the launch:
                              # 256 when the stack's matrices make more than 1024 tiles of 128 (more than the 768 block slots
                              # hold at once), else 128.  Measured: arch.vqvae-ema (768 tiles) 1.66 ms with 128, 2.21 ms with
                              # 256 - a lone block fills its LDS at ~26 GB/s whatever its ring depth, three independent blocks
                              # per CU reach 43 GB/s together; the deep decoder (30 x 512: 1450 tiles, bound by what it
                              # re-fetches) 67.1 ms per step with 128, 64.8 with 128 + row cursor, 62.9 with 256
                              # (profiles/r04_notes.md 24, 25)
    wgrad_cursor = None       # the grouped weight-gradient launches of the stack paced by the row cursor
                              # (aew_gemm_tn_group_t.cursors): True / False / None = iff the launch has more tiles than
                              # TnGroupBuilder.CURSOR_AUTO_TILES.  Measured: arch.vqvae-ema (768 tiles, one resident wave) 7.03 ->
                              # 7.26 ms per step although the launch fetches 28 % less - it is not bound by what it fetches;
                              # the deep decoder (30 x 512, 1450 tiles of 268 k rows) 66.5 -> 64.4 ms (weight-gradient class
                              # 24.9 -> 23.0 ms) - there it is (profiles/r04_notes.md 21, 24)
    split_chains_bwd = False  # the backward's dz / dx chain as two half-batch chains on lanes 4 / 5 (see split_chains)
    tail_lane = 0             # 4: the LAST grouped weight-gradient launch, the speaker / gated-bias gradients that read its column
                              # sums and the decoder's gradient unpack form one side branch on this lane (lane mode 2 honours
                              # lanes 4 / 5 alone; TrainEngine.graph_lanes), and everything else after the dgrad chain - cond
                              # gradient, upsampler / LC backward, bottleneck and encoder backward: ~0.6 ms of small launches
                              # that depend on no weight gradient - runs beside it on the main lane: ONE fork after dx.0, one
                              # join before the last unpack.  Measured on three boxes, interleaved: 6.83 vs 6.91, 6.99 vs 6.97,
                              # 6.99 vs 6.90 ms per step - the grouped launch holds three blocks on most CUs for its whole 1.6
                              # ms, so the small launches only get the leftover slots, and the fork / join costs what that
                              # returns (profiles/r04_notes.md 18).  0 (default): serial plan order
    wgrad_split_layers = 0    # with grouped wgrads: the TOP this-many layers keep one split-K TN op per matrix (they run
                              # under the dgrad chain and fill its tile-wave tails), the rest go to the grouped launch
    ups_split_rows = 1024     # upsampler / lc-conv weight gradients (few output tiles): contractions longer than this many
                              # rows x batch are cut into 512-row chunks (one block and one slab each) in the grouped launch
    split_one_lane = False    # with split_chains / split_chains_bwd: both half-batch chains on the MAIN lane, interleaved stage by
                              # stage - no graph branches; meant for the chained launch (TrainEngine.nt_chain), where the stages of
                              # the two halves then alternate inside ONE launch and each half's tiles run while the other half's
                              # wait for their producers
    split_chains = False      # True: gated stack as two half-batch chains on lanes 4 / 5 (build_forward); split_chains_bwd: the
                              # same for the backward's dz / dx chain.  Captured as graph branches (TrainEngine.graph_lanes) both
                              # together return 0.07-0.125 ms per step (five boxes, interleaved: 6.95 -> 6.85, 6.97 -> 6.905,
                              # 6.98 -> 6.885, 6.85 -> 6.755, 6.945 -> 6.82; either one alone: -0.09 ... +0.03), bit-identical
                              # results (tests/test_gpu_parity.py).  Default off: two concurrent half-batch launches each run
                              # longer than half a full-batch launch, so every per-kernel duration - HIP events in serial
                              # timing mode, rocprofv3 under overlap - and with it the roofline line of bench.py would stop
                              # describing the kernel; 1.5 % of the step is less than the box-to-box spread (profiles/r04_notes.md 19)

    def __init__(self, ws: Workspace, ps: ParamStore, hps, geom: G.ModelGeom, B: int, pre: str,
                 n_lc_in: int, lc_src: Mat, wav: torch.Tensor, voice: torch.Tensor,
                 jitter: torch.Tensor, take_compat: bool, packer: Packer, impl: int = 0,
                 wgrad_group: Optional[int] = None):
        self.ws, self.ps, self.hps, self.g, self.B, self.pre = ws, ps, hps, geom, B, pre
        self.impl = impl
        import os as _os
        if _os.environ.get("AEW_FN_OPS") is not None:          # A/B aid: comma list, "" = none
            self.fn_ops = frozenset(v for v in _os.environ["AEW_FN_OPS"].split(",") if v)
        if wgrad_group is not None:                            # resolved once by TrainEngine (argument, else AEW_WGRAD_GROUP,
            self.wgrad_group = int(wgrad_group)                # else the class default) and shared with the EncoderPlan
        if hps.n_global_embed > 16:
            # k_spk_bwd holds a layer's speaker-projection row in registers (AEW_SPK_MAXG)
            raise ValueError(f"n_global_embed = {hps.n_global_embed}: the speaker-gradient kernel supports at most 16")
        self.gmul_ptr = ws.bufs["loss.gmul"].data_ptr() if "loss.gmul" in ws.bufs else 0
        self.n_lc_in = n_lc_in
        self.lc_src, self.wav, self.voice, self.jitter = lc_src, wav, voice, jitter
        self.take_compat = take_compat
        self.pk = packer
        h = hps
        self.R, self.D, self.S, self.P, self.Q = h.n_res, h.n_dil, h.n_skp, h.n_post, h.n_quant
        self.Clc, self.Gc = h.n_lc_out, h.n_global_embed
        self.Rp, self.Dp, self.Sp, self.Pp, self.Qp = (ru(v, 128) for v in (self.R, self.D, self.S, self.P, self.Q))
        self.Cp, self.Lp = ru(self.Clc, 128), ru(n_lc_in, 128)
        self.NL = len(geom.layers)
        self.T, self.w = geom.dec_in_len, geom.n_win
        self.Ne = geom.embed_len
        self.peak_ptrs = None               # (per-position peak log-probability, arg-max) the forward softmax writes (set by TrainEngine)
        self.unpack_early_tbl: Optional[CopyTableBuilder] = None    # build_backward's early table, as given
        self.hi_first_layer: Optional[int] = None   # build_backward: layers from here up are final mid-chain (WgradRouter)
        self.tail_lane_used, self._lane_rr = 0, 0   # build_backward: tail_lane as applied; _next_lane's rotation
        self._alloc()
        self._pack_records()

    # -- buffers --------------------------------------------------------------------------
    def _alloc(self):
        ws, B, g = self.ws, self.B, self.g
        p = self.pre
        M = lambda n, rows, pitch, dt, cols=None, guard=0: Mat.new(ws, p + n, B, rows, pitch, dt, cols, guard)
        self.lcj = M("lcj", self.Ne, self.Lp, BF)
        self.lc_lens = g.lc_lens                      # [Ne, Ne-2, after each upsampler]
        self.ups_in: List[Mat] = [M("lc1", self.lc_lens[1], self.Cp, BF)]
        n_ups = len(self.hps.lc_upsample_strides)
        # upsampler outputs carry guard rows: the merged-phase GEMM writes `stride` matrix rows per GEMM row
        for i in range(n_ups - 1):
            self.ups_in.append(M(f"ups{i}", self.lc_lens[2 + i], self.Cp, BF, guard=8))
        self.cond = M("cond", self.T, self.Cp, BF, guard=8)
        self.bias_bl = ws.alloc(p + "bias_bl", B * self.NL * 2 * self.Dp, torch.float32)
        self.gc = ws.alloc(p + "gc", B * self.Gc, torch.float32)
        self.x: List[Mat] = [M(f"x{l}", lg.in_len, self.Rp, BF) for l, lg in enumerate(g.layers)]
        self.z = [M(f"z{l}", lg.out_len, self.Dp, BF) for l, lg in enumerate(g.layers)]
        # local derivatives dz/dfilt, dz/dgate saved by the gated epilogue for backward
        self.pf = [M(f"pf{l}", lg.out_len, self.Dp, BF) for l, lg in enumerate(g.layers)]
        self.pg = [M(f"pg{l}", lg.out_len, self.Dp, BF) for l, lg in enumerate(g.layers)]
        self.h0 = M("h0", self.w, self.Sp, BF)
        self.skp_part = M("skp_part", self.w, self.Sp, BF)      # skip sum of the lower half of the stack (pre-relu)
        self.h1 = M("h1", self.w, self.Pp, BF)
        self.logits = M("logits", self.w, self.Qp, F3)
        self.nll = ws.alloc(p + "nll", B * self.w, torch.float32)
        self.ptgt = ws.alloc(p + "ptgt", B * self.w, torch.float32)
        # backward
        self.onehot = M("onehot", self.T, self.Qp, BF)
        self.dlogits = M("dlogits", self.w, self.Qp, BF)
        self.dh1 = M("dh1", self.w, self.Pp, BF)
        self.dskp = M("dskp", self.w, self.Sp, BF)
        # one dx buffer per layer (not a ping-pong pair): the res / base wgrads that read dx_{l+1} run
        # on the side lane and may lag the dx chain by several layers
        self.dx = [M(f"dx{l}", g.layers[l].in_len, self.Rp, BF) for l in range(self.NL)]
        self.dfg = [M(f"dfg{l}", lg.out_len, 2 * self.Dp, BF) for l, lg in enumerate(g.layers)]
        self.colsum_fg = ws.alloc(p + "colsum_fg", B * self.NL * 2 * self.Dp, torch.float32)
        self.dcond = M("dcond", self.T, self.Cp, BF)
        self.dcond_part = M("dcond_part", self.T, self.Cp, BF)  # cond gradient of the upper half of the stack
        self.dups = [M(f"d{m.name[len(p):]}", m.rows, self.Cp, BF) for m in self.ups_in]
        self.dlcj = M("dlcj", self.Ne, self.Lp, F3)
        # gradient w.r.t. the LC source (fp32, same shape as lc_src)
        self.dlc_src = Mat.new(ws, p + "dlc_src", B, self.lc_src.rows, self.lc_src.pitch, F3)
        # offset tables for the speaker-bias ops
        offs = {k: [] for k in ("bs", "bg", "ps", "pg")}
        for l in range(self.NL):
            q = p + f"conv_layers.{l}."
            offs["bs"].append(self.ps.off.get(q + "conv_signal.bias", -1))
            offs["bg"].append(self.ps.off.get(q + "conv_gate.bias", -1))
            offs["ps"].append(self.ps.off[q + "proj_signal.weight"])
            offs["pg"].append(self.ps.off[q + "proj_gate.weight"])
        self.off_tbl = {}
        for k, v in offs.items():
            t = ws.alloc(p + "off_" + k, self.NL, torch.int64)
            t[:self.NL].copy_(torch.tensor(v, dtype=torch.int64))
            self.off_tbl[k] = t

    def _impl(self, kind: str) -> int:
        """impl of an NT op of the given kind: the full-N kernels (2) where selected, unless the engine was built on
        the scalar check kernels (impl 1)."""
        return 2 if (self.impl == 0 and kind in self.fn_ops) else self.impl

    def _wmat(self, name, rows, cols, dt=BF) -> Mat:
        return Mat.new(self.ws, self.pre + "wp." + name, 1, rows, cols, dt)

    def _chains(self, plan: Plan, n_chains: int):
        """One stage of n_chains half-batch chains: per chain c sets its lane - 4 + c, unless split_one_lane interleaves two
        chains on the main lane - and yields (c, first batch element, label suffix); back on the main lane afterwards."""
        for c in range(n_chains):
            plan.lane = (4 + c) if (n_chains > 1 and not self.split_one_lane) else 0
            yield c, c * (self.B // n_chains), (f".c{c}" if n_chains > 1 else "")
        plan.lane = 0

    # -- packed weight matrices and their pack/unpack records ------------------------------
    def _pack_records(self):
        pk, p, ps = self.pk, self.pre, self.ps
        R, D, S, P, Q, Clc = self.R, self.D, self.S, self.P, self.Q, self.Clc
        Rp, Dp, Sp, Pp, Qp, Cp, Lp = self.Rp, self.Dp, self.Sp, self.Pp, self.Qp, self.Cp, self.Lp
        Cc = Clc + self.Gc
        NL = self.NL
        self.Wfg, self.Wrs, self.WrsT, self.WfgT = [], [], [], []
        # name of a weight gradient -> the pieces of the packed matrix whose layout its slab has (packed here, unpacked
        # by build_backward from the same pieces)
        self.lay: Dict[str, List[Piece]] = {}
        Kfg = 2 * Rp + Cp
        # the 20-segment GEMMs (skip sum, cond gradient) run as two halves: the half whose inputs exist
        # mid-chain goes to a side lane (fills tile-wave tails), the other half adds it as aux
        self.n_lo = NL // 2 if (self.split_multiseg and NL >= 4) else NL      # layers [0, n_lo) | [n_lo, NL)
        n_lo, n_hi = self.n_lo, NL - self.n_lo
        self.VfgT_lo = self._wmat("VfgT_lo", Cp, n_lo * 2 * Dp)
        self.VfgT_hi = self._wmat("VfgT_hi", Cp, max(n_hi, 1) * 2 * Dp)
        self.Wskp_lo = self._wmat("skp_lo", Sp, n_lo * Dp)
        self.Wskp_hi = self._wmat("skp_hi", Sp, max(n_hi, 1) * Dp)
        # base layer as a row gather: transposed fp32 copy [Q][Rp] (wavenet.py:348-351).  (Its gradient comes out of a TN
        # GEMM over the one-hot matrix as [Rp][Qp], not in this layout: build_backward states that map itself.)
        self.Wbase_t = self._wmat("base_t", Q, Rp, F3)
        pk.pack(Piece(p + "base_layer.weight", 0, [Q, 1], [R, Q], 0, [1, Rp]), self.Wbase_t)
        for l in range(NL):
            last = l == NL - 1
            q = p + f"conv_layers.{l}."
            Wfg = self._wmat(f"fg{l}", 2 * Dp, Kfg)
            WfgT = self._wmat(f"fgT{l}", Rp, 4 * Dp)
            self.Wfg.append(Wfg); self.WfgT.append(WfgT)
            Vt, lv, nv = (self.VfgT_lo, l, n_lo) if l < n_lo else (self.VfgT_hi, l - n_lo, n_hi)
            fg = self.lay[f"fg{l}"] = []
            for gate, nm in ((0, "signal"), (1, "gate")):
                for co0, ng, gl in _gate_groups(D):
                    row0 = (co0 // 16) * 32 + 16 * gate
                    # conv weight [D][R][2] -> Wfg rows, tap-major K; and WfgT (dgrad) layout
                    conv = Piece(q + f"conv_{nm}.weight", co0 * R * 2, [16 * R * 2, R * 2, 2, 1], [ng, gl, R, 2],
                                 row0 * Kfg, [32 * Kfg, Kfg, 1, Rp])
                    # conditioning projection [D][Cc][1], first Clc columns only
                    proj = Piece(q + f"proj_{nm}.weight", co0 * Cc, [16 * Cc, Cc, 1], [ng, gl, Clc],
                                 row0 * Kfg + 2 * Rp, [32 * Kfg, Kfg, 1])
                    fg += [conv, proj]
                    pk.pack(conv, Wfg)
                    pk.pack(conv.at(row0, [32, 1, 4 * Dp, 2 * Dp]), WfgT)
                    pk.pack(proj, Wfg)
                    pk.pack(proj.at(lv * 2 * Dp + row0, [32, 1, nv * 2 * Dp]), Vt)
            # residual 1x1 (forward) and [res | skip]^T (backward dz); the skip 1x1s of ALL layers
            # form one matrix Wskp [Sp][NL*Dp] for the deferred skip GEMM (wavenet.py:103,357)
            Nrs = Sp if last else Rp + Sp
            Wrs = None if last else self._wmat(f"rs{l}", Rp, Dp)
            WrsT = self._wmat(f"rsT{l}", Dp, Nrs)
            self.Wrs.append(Wrs); self.WrsT.append(WrsT)
            if not last:
                res = Piece(q + "dil_res.weight", 0, [D, 1], [R, D], 0, [Dp, 1])
                self.lay[f"res{l}"] = [res]
                pk.pack(res, Wrs)
                pk.pack(res.at(0, [1, Nrs]), WrsT)
            # (the skip gradient spans all NL layers in ONE matrix whatever split_multiseg does to the packed pair:
            # _skip_piece states its map)
            Ws, ls, ns = (self.Wskp_lo, l, n_lo) if l < n_lo else (self.Wskp_hi, l - n_lo, n_hi)
            skp = self._skip_piece(l, ls, ns)
            pk.pack(skp, Ws)
            pk.pack(skp.at(0 if last else Rp, [1, Nrs]), WrsT)
        # post network
        self.Wp1, self.Wp1T = self._wmat("p1", Pp, Sp), self._wmat("p1T", Sp, Pp)
        self.Wp2, self.Wp2T = self._wmat("p2", Qp, Pp), self._wmat("p2T", Pp, Qp)
        p1 = Piece(p + "post1.weight", 0, [S, 1], [P, S], 0, [Sp, 1])
        p2 = Piece(p + "post2.weight", 0, [P, 1], [Q, P], 0, [Pp, 1])
        self.lay["p1"], self.lay["p2"] = [p1], [p2]
        pk.pack(p1, self.Wp1)
        pk.pack(p1.at(0, [1, Pp]), self.Wp1T)
        pk.pack(p2, self.Wp2)
        pk.pack(p2.at(0, [1, Qp]), self.Wp2T)
        # fp32 bias vectors padded to N_pad
        self.bias_vec: Dict[str, int] = {}
        for nm, n, npad in (("post1", P, Pp), ("post2", Q, Qp), ("lc_conv", Clc, Cp)):
            t = self.ws.alloc(p + "wp.bias." + nm, npad, torch.float32)
            self.bias_vec[nm] = t.data_ptr()
            if ps.has(p + nm + ".bias"):
                pk.pack_tbl.add(ps.ptr(p + nm + ".bias"), t.data_ptr(), [n], [1], [1], F3, F3)
        # LC conv [Clc][n_lc_in][3]
        nin = self.n_lc_in
        self.Wlc, self.WlcT = self._wmat("lc", Cp, 3 * Lp), self._wmat("lcT", Lp, 3 * Cp)
        lc = Piece(p + "lc_conv.weight", 0, [nin * 3, 3, 1], [Clc, nin, 3], 0, [3 * Lp, 1, Lp])
        self.lay["lc"] = [lc]
        pk.pack(lc, self.Wlc)
        pk.pack(lc.at(0, [1, 3 * Cp, Cp]), self.WlcT)
        # upsamplers: ConvTranspose1d weight [ci][co][k]
        self.Wup, self.Wup_all, self.WupT = [], [], []          # per stage: [phase matrices], all phases as one, dgrad layout
        for i, (f, s) in enumerate(zip(self.hps.lc_upsample_filt_sizes, self.hps.lc_upsample_strides)):
            nm = p + f"lc_upsample.{i}.tconv.weight"
            phases = []
            Kph = (f // s) * Cp
            Wall = self._wmat(f"up{i}", s * Cp, Kph)             # phase ph = rows ph*Cp .. (ph+1)*Cp
            for ph in range(s):
                Wm = Mat(self.ws, Wall.name, 1, Cp, Kph, BF, base_off=ph * Cp * Kph)
                # [co][j*Cp + ci] <- W[ci][co][ph + s*j]
                pk.pack(Piece(nm, ph, [f, Clc * f, s], [Clc, Clc, f // s], 0, [(f // s) * Cp, 1, Cp]), Wm)
                phases.append(Wm)
            self.Wup.append(phases)
            self.Wup_all.append(Wall)
            WT = self._wmat(f"upT{i}", Cp, f * Cp)
            # [ci][k*Cp + co] <- W[ci][co][k]: the dgrad matrix, and the layout of the weight gradient
            up = Piece(nm, 0, [Clc * f, f, 1], [Clc, Clc, f], 0, [f * Cp, 1, Cp])
            self.lay[f"up{i}"] = [up]
            pk.pack(up, WT)
            self.WupT.append(WT)
            t = self.ws.alloc(p + f"wp.bias.up{i}", s * Cp, torch.float32)     # the bias once per phase
            self.bias_vec[f"up{i}"] = t.data_ptr()
            for ph in range(s):
                pk.pack_tbl.add(ps.ptr(p + f"lc_upsample.{i}.tconv.bias"), t.data_ptr() + 4 * ph * Cp, [Clc], [1], [1],
                                F3, F3)

    def _skip_piece(self, l: int, col_layer: int, n_layers: int) -> Piece:
        """dil_skp of layer l as columns [col_layer * Dp, +D) of a skip matrix that holds n_layers layers side by side."""
        return Piece(self.pre + f"conv_layers.{l}.dil_skp.weight", 0, [self.D, 1], [self.S, self.D],
                     col_layer * self.Dp, [n_layers * self.Dp, 1])

    # -- forward ---------------------------------------------------------------------------
    def build_forward(self, plan: Plan, need_onehot: bool = True, after_logits=None, after_nll=None):
        """after_logits / after_nll: callables(plan) that append side-lane ops reading the logits / the per-position
        nll (the caller's per-step diagnostics): placed here they run under the softmax and the loss reduction
        instead of after the plan's last main-lane op."""
        B, g, hps, p = self.B, self.g, self.hps, self.pre
        Rp, Dp, Sp, Pp, Qp, Cp, Lp = self.Rp, self.Dp, self.Sp, self.Pp, self.Qp, self.Cp, self.Lp
        impl = self.impl
        # 4./5. (emitted FIRST when side_inputs_first: they depend on nothing in this plan, so the side lane runs them
        # under the conditioning path instead of starting after its last op)
        def side_inputs():
            # 4. speaker-conditioned gated bias (wavenet.py:127-140 folded)
            sb = L.SpkBias()
            self._fill_spk(sb)
            sb.bias, sb.gc = self.bias_bl.data_ptr(), self.gc.data_ptr()
            with plan.side():                                      # independent of the conditioning path
                plan.add(L.OP_SPK_BIAS, sb, "spk_bias", TAG_MISC)
            # 5. base layer = column gather (wavenet.py:348-351)
            bg = L.BaseGather()
            bg.wav, bg.wav_pitch, bg.wav_off = self.wav.data_ptr(), self.wav.shape[1], g.trim_dec_in[0]
            bg.W = self.ps.ptr(p + "base_layer.weight")
            bg.Wt = self.Wbase_t.ptr
            bg.bias = self.ps.ptr(p + "base_layer.bias") if self.ps.has(p + "base_layer.bias") else None
            bg.B, bg.T, bg.R, bg.R_pad, bg.Q = B, self.T, self.R, Rp, self.Q
            bg.x, bg.x_bs, bg.x_pitch = self.x[0].ptr, self.x[0].bs, self.x[0].pitch
            if need_onehot:
                bg.onehot, bg.oh_bs, bg.oh_pitch, bg.Q_pad = self.onehot.ptr, self.onehot.bs, self.onehot.pitch, Qp
            bg.ones_channel = int(self.R < Rp)
            with plan.side():
                plan.add(L.OP_BASE_GATHER, bg, "base_gather", TAG_MISC)
        if self.side_inputs_first:
            side_inputs()
        # 1. jitter gather (wavenet.py:330-336)
        lg_ = L.LcGather()
        lg_.src, lg_.src_bs, lg_.src_pitch = self.lc_src.ptr, self.lc_src.bs, self.lc_src.pitch
        lg_.jitter, lg_.jit_pitch = self.jitter.data_ptr(), self.jitter.shape[1]
        lg_.dst, lg_.dst_bs, lg_.dst_pitch = self.lcj.ptr, self.lcj.bs, self.lcj.pitch
        lg_.B, lg_.N, lg_.C, lg_.C_pad = B, self.Ne, self.n_lc_in, Lp
        lg_.take_compat = int(self.take_compat)
        plan.add(L.OP_LC_GATHER, lg_, "lc_gather", TAG_UPS)
        # 2. LC conv k=3 (wavenet.py:337)
        lc1 = self.ups_in[0]
        plan.add(L.OP_GEMM_NT, make_nt(
            BF, lc1.rows, Cp, Cp, B, [self.lcj.seg(Lp, row_off=t) for t in range(3)], self.Wlc.ptr,
            flags=L.EF_BIAS, out0=lc1.view(), bias_ptr=self.bias_vec["lc_conv"], impl=impl), "lc_conv", TAG_UPS)
        # 3. transposed-conv upsamplers as polyphase GEMMs (wavenet.py:154,338)
        n_ups = len(hps.lc_upsample_strides)
        for i, (f, s) in enumerate(zip(hps.lc_upsample_filt_sizes, hps.lc_upsample_strides)):
            X = self.ups_in[i]
            Lin, Lout, pad = X.rows, self.lc_lens[2 + i], f - s
            last = i == n_ups - 1
            trim0 = g.trim_ups_out[0] if last else 0
            Y = self.cond if last else self.ups_in[i + 1]
            if pad % s == 0 and f % s == 0 and s <= 8:
                # all phases in ONE GEMM: N = s*Cp, GEMM row q holds matrix rows s*q + ph - trim0 (ph = 0..s-1),
                # i.e. the output is addressed as [rows/s][s*Cp]; partial rows at the ends land in the guard rows
                q0 = pad // s
                q_lo = trim0 // s
                q_hi = min(-(-(Y.rows + trim0) // s), (Lout - 1) // s + 1)
                Mq = q_hi - q_lo
                assert s * q_lo - trim0 >= -8 and s * (q_hi - 1) + s - 1 - trim0 < Y.rows + 8
                segs = [X.seg(Cp, row_off=q0 + q_lo - j) for j in range(f // s)]
                ov = L.View()
                ov.ptr = Y.ptr + 2 * (s * q_lo - trim0) * Cp
                ov.batch_stride, ov.row_pitch, ov.row_step, ov.row_off = Y.bs, s * Cp, 1, 0
                ov.row_lo, ov.row_hi, ov.dtype = 0, Mq, BF
                plan.add(L.OP_GEMM_NT, make_nt(
                    BF, Mq, s * Cp, s * Cp, B, segs, self.Wup_all[i].ptr, flags=L.EF_BIAS, out0=ov,
                    bias_ptr=self.bias_vec[f"up{i}"], impl=impl), f"ups{i}", TAG_UPS)
                continue
            for ph in range(s):
                q0 = -((ph - pad) // s)                 # ceil((pad - ph)/s): first q with o >= 0
                o0 = s * q0 + ph - pad
                if o0 >= Lout:
                    continue
                Mq = (Lout - 1 - o0) // s + 1
                segs = [X.seg(Cp, row_off=q0 - j) for j in range(f // s)]
                plan.add(L.OP_GEMM_NT, make_nt(
                    BF, Mq, Cp, Cp, B, segs, self.Wup[i][ph].ptr, flags=L.EF_BIAS,
                    out0=Y.view(row_off=o0 - trim0, row_step=s), bias_ptr=self.bias_vec[f"up{i}"],
                    impl=impl), f"ups{i}.ph{ph}", TAG_UPS)
        if not self.side_inputs_first:
            side_inputs()
        # 6. gated dilated stack (wavenet.py:91-111, 355-357)
        NL = self.NL
        # layer 0 waits for lane 1 only (x[0], gated biases), not for the other lanes' work that only later steps read
        g1_join = ("lane", 1) if self.side_inputs_first else True
        # Optionally (split_chains) the gated stack runs as two independent half-batch chains, chain 0 on the
        # main lane and chain 1 on the side lane, so that each fills the other's tile-wave tails (a full-batch
        # layer GEMM is 1.1-1.5 waves of tiles and nothing else is runnable in the forward).
        n_chains = 2 if (self.split_chains and B % 2 == 0 and B >= 2) else 1
        nb = B // n_chains
        for l, lg in enumerate(g.layers):
            last = l == NL - 1
            x = self.x[l]
            P_l = lg.out_len
            for c, b0, sfx in self._chains(plan, n_chains):
                # two chains: BOTH on side lanes (4 and 5: the ones aew_set_lanes(2) honours alone).  A side op is ordered after every main-lane op emitted before
                # it, so a chain left on the main lane would hold the other one back at every layer; with no main-lane op
                # between the first layer and the skip sum the two lanes run free
                segs = [x.seg(Rp, b0=b0), x.seg(Rp, row_off=lg.dil, b0=b0),
                        self.cond.seg(Cp, row_off=lg.cond_lead, b0=b0)]
                gkw = dict(epi=L.EPI_GATED, out0=self.z[l].view(b0=b0), out1=self.pf[l].view(b0=b0),
                           out2=self.pg[l].view(b0=b0),
                           bias_ptr=self.bias_bl.data_ptr() + 4 * (l * 2 * Dp + b0 * NL * 2 * Dp), bias_bs=NL * 2 * Dp)
                if not last and self._impl("layer") == 2:
                    # the gated pair as ONE op (wavenet.py:100-109): z never leaves the CU between the two GEMMs
                    plan.add(L.OP_GEMM_NT, make_nt(
                        BF, P_l, Dp, 2 * Dp, nb, segs, self.Wfg[l].ptr, impl=2, W2_ptr=self.Wrs[l].ptr, N2=Rp, N2_pad=Rp,
                        out3=self.x[l + 1].view(b0=b0), aux0=x.view(row_off=lg.dil, b0=b0), **gkw),
                        f"G1.{l}" + sfx, TAG_G1, join=g1_join if (l == 0 and c == 0) else False)
                    continue
                plan.add(L.OP_GEMM_NT, make_nt(
                    BF, P_l, Dp, 2 * Dp, nb, segs, self.Wfg[l].ptr, impl=self._impl("G1"), **gkw),
                    f"G1.{l}" + sfx, TAG_G1,
                    join=((g1_join if c == 0 else False) if self.split_one_lane else (True if n_chains > 1 else g1_join))
                    if l == 0 else False)                              # x[0] and the gated biases come from the side lane
                if not last:
                    # residual 1x1 + add (wavenet.py:108-109); the final layer has no residual output
                    plan.add(L.OP_GEMM_NT, make_nt(
                        BF, P_l, Rp, Rp, nb, [self.z[l].seg(Dp, b0=b0)], self.Wrs[l].ptr, flags=L.EF_ADD_AUX0,
                        out0=self.x[l + 1].view(b0=b0), aux0=x.view(row_off=lg.dil, b0=b0), impl=impl),
                        f"G2.{l}" + sfx, TAG_G2)
            if self.n_lo < NL and l == self.n_lo - 1:
                # early half of the skip sum (layers 0 .. n_lo-1): all its inputs exist now
                plan.lane = 0
                segs = [self.z[k].seg(Dp, row_off=g.layers[k].skip_lead) for k in range(self.n_lo)]
                with plan.side(self.EARLY_LANE):
                    plan.add(L.OP_GEMM_NT, make_nt(BF, self.w, Sp, Sp, B, segs, self.Wskp_lo.ptr,
                                                   out0=self.skp_part.view(), impl=impl), "skip_lo", TAG_G2,
                             join=n_chains > 1)
        plan.lane = 0
        # skip path of all layers as ONE GEMM: relu(sum_l Wk_l . z_l[u + skip_lead_l]) -> h0
        # (wavenet.py:103,355-359).  K = NL*256; the fp32 skip sum never touches HBM.
        # With split_multiseg the layers [0, n_lo) were already summed on a side lane right after
        # G1 of layer n_lo-1 (skp_part, below in the layer loop); this GEMM adds them and applies the relu.
        lo = self.n_lo
        if lo < NL:
            segs = [self.z[l].seg(Dp, row_off=g.layers[l].skip_lead) for l in range(lo, NL)]
            plan.add(L.OP_GEMM_NT, make_nt(BF, self.w, Sp, Sp, B, segs, self.Wskp_hi.ptr,
                                           flags=L.EF_ADD_AUX0 | L.EF_RELU_POST, out0=self.h0.view(),
                                           aux0=self.skp_part.view(), impl=self._impl("skip")), "skip_all", TAG_G2, join=True)
        else:
            segs = [self.z[l].seg(Dp, row_off=lg.skip_lead) for l, lg in enumerate(g.layers)]
            plan.add(L.OP_GEMM_NT, make_nt(BF, self.w, Sp, Sp, B, segs, self.Wskp_lo.ptr, flags=L.EF_RELU,
                                           out0=self.h0.view(), impl=self._impl("skip")), "skip_all", TAG_G2, join=True)
        # 7. post network (wavenet.py:359-360)
        plan.add(L.OP_GEMM_NT, make_nt(BF, self.w, Pp, Pp, B, [self.h0.seg(Sp)], self.Wp1.ptr,
                                       flags=L.EF_BIAS | L.EF_RELU, out0=self.h1.view(),
                                       bias_ptr=self.bias_vec["post1"], impl=self._impl("post")), "post1", TAG_POST)
        plan.add(L.OP_GEMM_NT, make_nt(BF, self.w, Qp, Qp, B, [self.h1.seg(Pp)], self.Wp2.ptr,
                                       flags=L.EF_BIAS, out0=self.logits.view(),
                                       bias_ptr=self.bias_vec["post2"], impl=impl), "post2", TAG_POST)
        if after_logits is not None:
            after_logits(plan)
        # 8. fused log-softmax + NLL (wavenet.py:543-547)
        plan.add(L.OP_SOFTMAX_NLL, self._softmax(False, 0.0), "softmax_nll", TAG_LOSS)
        if after_nll is not None:
            after_nll(plan)

    def _fill_spk(self, sb):
        p, ps = self.pre, self.ps
        sb.params, sb.voice = ps.params.data_ptr(), self.voice.data_ptr()
        sb.off_bias_sig, sb.off_bias_gate = self.off_tbl["bs"].data_ptr(), self.off_tbl["bg"].data_ptr()
        sb.off_proj_sig, sb.off_proj_gate = self.off_tbl["ps"].data_ptr(), self.off_tbl["pg"].data_ptr()
        sb.off_spk_w = ps.off[p + "cond.speaker_embedding.weight"]
        sb.off_spk_b = ps.off.get(p + "cond.speaker_embedding.bias", -1)
        sb.B, sb.L, sb.D, sb.D_pad, sb.C_lc, sb.G = self.B, self.NL, self.D, self.Dp, self.Clc, self.Gc
        sb.n_speakers = self.hps.n_speakers

    def _softmax(self, backward: bool, scale: float) -> L.SoftmaxNll:
        sm = L.SoftmaxNll()
        sm.logits, sm.bs, sm.pitch = self.logits.ptr, self.logits.bs, self.logits.pitch
        sm.wav, sm.wav_pitch, sm.tgt_off = self.wav.data_ptr(), self.wav.shape[1], self.g.wav_out_off
        sm.B, sm.w, sm.Q, sm.Q_pad = self.B, self.w, self.Q, self.Qp
        sm.nll, sm.ptgt = self.nll.data_ptr(), self.ptgt.data_ptr()
        sm.dlogits, sm.dl_bs, sm.dl_pitch = self.dlogits.ptr, self.dlogits.bs, self.dlogits.pitch
        sm.scale, sm.backward = scale, int(backward)
        if not backward and self.peak_ptrs:
            sm.peak, sm.amax = self.peak_ptrs
        if backward and self.gmul_ptr:
            sm.gmul = self.gmul_ptr
        return sm

    # -- backward --------------------------------------------------------------------------
    def _colsum(self, plan: Plan, X: Mat, M: int, N: int, out_ptr: int, out_bs: int = 0, label: str = "colsum"):
        cs = colsum_op(self.ws, X.seg(128), X.dtype, M, N, self.B, out_ptr, out_bs, self.pre + "det." + label)
        with plan.side(self._next_lane()):
            plan.add(L.OP_COLSUM, cs, label, TAG_MISC)

    def _next_lane(self) -> int:
        n = min(self.n_side_lanes, Plan.N_SIDE, 3)             # lanes 4 / 5 are for explicit branches (tail_lane, split_chains)
        self._lane_rr = self._lane_rr % max(1, n) + 1
        return self._lane_rr

    def _tn(self, Mc: int, N: int, N_pad: int, gseg: L.Seg, segs: Sequence[L.Seg]) -> L.GemmTN:
        return make_tn(BF, Mc, self.B, N, N_pad, gseg, segs, impl=self.impl)

    def _spk_bwd(self, first: int, count: int, running: int, det_tag: str) -> "L.SpkBwd":
        """Speaker-embedding / gated-bias gradients of layers [first, first + count) (count 0: all) from colsum_fg, whose
        first `running` layers hold running sums over the batch (the grouped launch's snapshots)."""
        sb = L.SpkBwd()
        self._fill_spk(sb)
        sb.colsum, sb.gc, sb.grads = self.colsum_fg.data_ptr(), self.gc.data_ptr(), self.ps.grads.data_ptr()
        sb.colsum_running = running
        if count:
            sb.layer_range = first | (count << 16)
        # scratch + ticket of the deterministic speaker-embedding sums (aew_spk_bwd_t.det_scratch: one [16][16] block of terms
        # per (layer, filt | gate, chunk of 16 batch elements), added in a fixed order by the last block)
        chunks = (self.B + 15) // 16
        sb.det_scratch = self.ws.alloc(self.pre + f"det.spk_{det_tag}.scratch", self.NL * 2 * chunks * 256, torch.float32).data_ptr()
        sb.det_tickets = self.ws.alloc(self.pre + f"det.spk_{det_tag}.tickets", 4, torch.int32, zero=True).data_ptr()
        return sb

    def build_backward(self, plan: Plan, nll_scale: float, early_tbl: Optional[CopyTableBuilder] = None):
        """nll_scale = d(loss)/d(per-position nll): 1/(B*(w-1)) for mean-type losses, 1 for sum-type (times the upstream
        gradient).  early_tbl: gradients of the post network and of the upper half of the stack are unpacked mid-chain by this table
        (side lane), so that less unpack work is left when the chain ends (shorter drain before the encoder backward /
        before a data-parallel caller may start reducing the decoder gradients); the caller emits the packer's own."""
        self.unpack_early_tbl, self.hi_first_layer = early_tbl, None
        rt = WgradRouter(self, plan, early_tbl)
        # split_chains_bwd: the dz / dx chain as two independent half-batch chains on lanes 4 / 5 (the mirror of the
        # forward's split_chains; ONE grouped weight-gradient launch only, so that nothing else sits inside the chain)
        n_chains = 2 if (self.split_chains_bwd and rt.grouped and not rt.multi and self.wgrad_split_layers == 0
                         and self.B % 2 == 0 and self.n_lo >= self.NL) else 1
        # (the tail branch is for the one-chain plan only: queued behind a chain on lane 4 it needs lanes 4 and 5 to wait
        # for each other in turn, and capturing that shape crashes inside the runtime - ROCm 7.2)
        tail = self.tail_lane_used = self.tail_lane if n_chains == 1 else 0
        self._bwd_post(plan, rt, nll_scale)
        dx0, colsum_tbl = self._bwd_stack(plan, rt, n_chains)
        self._bwd_base_skip(plan, rt, dx0, tail, n_chains)
        # tail_lane: the speaker / gated-bias gradients right behind the last grouped launch, before any main-lane op, so
        # that the branch needs no second edge from the main lane
        if tail:
            self._bwd_spk(plan, rt, colsum_tbl, tail)
        self._bwd_cond(plan, n_chains)
        if not tail:
            self._bwd_spk(plan, rt, colsum_tbl, tail)
        self._bwd_ups(plan, rt)

    def _bwd_post(self, plan: Plan, rt: "WgradRouter", nll_scale: float):
        """Loss gradient and post network (wavenet.py:359-360, 543-547)."""
        B, p, w, impl, Sp, Pp, Qp = self.B, self.pre, self.w, self.impl, self.Sp, self.Pp, self.Qp
        plan.add(L.OP_SOFTMAX_NLL, self._softmax(True, nll_scale), "softmax_grad", TAG_LOSS)
        plan.zero(self.ws, p + "colsum_fg")
        rt.add("p2", self._tn(w, self.Q, Qp, self.dlogits.seg(Qp), [self.h1.seg(Pp)]), TAG_POST, rt.LATE,
               bias=(p + "post2.bias", self.dlogits, "db.post2"))
        plan.add(L.OP_GEMM_NT, make_nt(BF, w, Pp, Pp, B, [self.dlogits.seg(Qp)], self.Wp2T.ptr, flags=L.EF_MUL_POS1,
                                       out0=self.dh1.view(), aux1=self.h1.view(), impl=impl), "d.post2", TAG_POST)
        rt.add("p1", self._tn(w, self.P, Pp, self.dh1.seg(Pp), [self.h0.seg(Sp)]), TAG_POST, rt.LATE,
               bias=(p + "post1.bias", self.dh1, "db.post1"))
        plan.add(L.OP_GEMM_NT, make_nt(BF, w, Sp, Sp, B, [self.dh1.seg(Pp)], self.Wp1T.ptr, flags=L.EF_MUL_POS1,
                                       out0=self.dskp.view(), aux1=self.h0.view(), impl=impl), "d.post1", TAG_POST)
        if rt.multi:
            self._bwd_skip_wgrad(rt)                           # into the first group: dskp and every z exist already

    def _bwd_skip_wgrad(self, rt: "WgradRouter"):
        """Skip weights of all layers: ONE wgrad with NL segments (mirror of the deferred skip GEMM):
        dW_skp[s][l*Dp + k] = sum_t dskp[t][s] * z_l[t + skip_lead_l][k].  640 tiles x batch fill the chip without row
        splits, so it writes B slabs instead of ~128 per layer.  The gradient always spans all NL layers, while the
        packed matrix may be two (split_multiseg): its per-layer map is stated here, not taken from the pack."""
        segs = [self.z[l].seg(self.Dp, row_off=self.g.layers[l].skip_lead) for l in range(self.NL)]
        rt.add("skp_all", self._tn(self.w, self.S, self.Sp, self.dskp.seg(self.Sp), segs), TAG_WG_RS, rt.LATE,
               pieces=[self._skip_piece(l, l, self.NL) for l in range(self.NL)])

    def _bwd_stack(self, plan: Plan, rt: "WgradRouter", n_chains: int) -> Tuple[Mat, CopyTableBuilder]:
        """Gated stack, last layer first: the dz / dx chain with each layer's weight gradients routed beside it.  Returns
        dx of layer 0 and the table that gathers per-batch column sums of dfg out of split-K weight gradients."""
        B, g, p, impl, NL = self.B, self.g, self.pre, self.impl, self.NL
        R, Rp, Dp, Sp, Cp = self.R, self.Rp, self.Dp, self.Sp, self.Cp
        Kfg = 2 * Rp + Cp
        dx_next: Optional[Mat] = None
        colsum_tbl = CopyTableBuilder(self.ws, p + "tbl.colsum")
        nb = B // n_chains
        for l in range(NL - 1, -1, -1):
            lg, last = g.layers[l], l == NL - 1
            P_l, d = lg.out_len, lg.dil
            for c, b0, sfx in self._chains(plan, n_chains):
                segs = ([] if last else [dx_next.seg(Rp, hi=P_l, b0=b0)]) + [self.dskp.seg(Sp, row_off=-lg.skip_lead, b0=b0)]
                plan.add(L.OP_GEMM_NT, make_nt(BF, P_l, Dp, Dp, nb, segs, self.WrsT[l].ptr, epi=L.EPI_DFG,
                                               aux0=self.pf[l].view(b0=b0), aux1=self.pg[l].view(b0=b0),
                                               out0=self.dfg[l].view(b0=b0), impl=self._impl("dz")), f"dz.{l}" + sfx, TAG_DZ)
            if self.n_lo < NL and l == self.n_lo:
                hsegs = [self.dfg[k].seg(2 * Dp, row_off=-g.layers[k].cond_lead) for k in range(self.n_lo, NL)]
                with plan.side(self.EARLY_LANE):               # upper half of the cond gradient: inputs complete
                    plan.add(L.OP_GEMM_NT, make_nt(BF, self.T, Cp, Cp, B, hsegs, self.VfgT_hi.ptr,
                                                   out0=self.dcond_part.view(), impl=impl), "dcond_hi", TAG_DCOND)
            x = self.x[l]
            if not last:
                rt.add(f"res{l}", self._tn(P_l, R, Rp, dx_next.seg(Rp, hi=P_l), [self.z[l].seg(Dp)]), TAG_WG_RS, l)
            t = self._tn(P_l, 2 * Dp, 2 * Dp, self.dfg[l].seg(2 * Dp),
                         [x.seg(Rp), x.seg(Rp, row_off=d), self.cond.seg(Cp, row_off=lg.cond_lead)])
            colsum_l = self.colsum_fg.data_ptr() + 4 * l * 2 * Dp
            if rt.in_group(l):
                # running per-batch column sums of dfg out of the grouped launch: column R of the weight gradient where x
                # carries the ones channel (R < Rp), else the launch's own all-ones operand (aew_gemm_tn_t.snap_k = -1)
                t.snap_out, t.snap_bs, t.snap_k = colsum_l, NL * 2 * Dp, (R if R < Rp else -1)
            wg = rt.add(f"fg{l}", t, TAG_WG_FG, l)
            spb = wg.slabs // B if (wg.slabs % B == 0 and wg.slabs >= B) else 0     # slabs per batch (0: batch folded)
            if rt.in_group(l):
                pass                                               # (its running column sums come from the grouped launch)
            elif R < Rp and spb > 0:
                # x carries a constant 1.0 in pad channel R (base_gather ones_channel), so column R
                # of this wgrad is sum_t dfg[t][n]: gather it per batch for the bias / speaker grads
                colsum_tbl.add(wg.ptr + 4 * R, colsum_l, [B, 2 * Dp], [spb * wg.stride, Kfg], [NL * 2 * Dp, 1], F3, F3,
                               red_n=spb, red_stride=wg.stride)
            else:
                self._colsum(plan, self.dfg[l], P_l, 2 * Dp, colsum_l, out_bs=NL * 2 * Dp, label=f"colsum.dfg{l}")
            rt.layer_done(l)
            dx = self.dx[l]
            for c, b0, sfx in self._chains(plan, n_chains):
                segs = [self.dfg[l].seg(2 * Dp, b0=b0), self.dfg[l].seg(2 * Dp, row_off=-d, b0=b0)]
                plan.add(L.OP_GEMM_NT, make_nt(
                    BF, lg.in_len, Rp, Rp, nb, segs, self.WfgT[l].ptr, flags=0 if last else L.EF_ADD_AUX0,
                    out0=dx.view(hi=lg.in_len, b0=b0), aux0=null_view() if last else dx_next.view(row_off=-d, hi=P_l, b0=b0),
                    impl=self._impl("dx")), f"dx.{l}" + sfx, TAG_DX)
            dx_next = dx
            rt.dx_done(l)
        return dx_next, colsum_tbl

    def _bwd_base_skip(self, plan: Plan, rt: "WgradRouter", dx0: Mat, tail: int, n_chains: int):
        """Base layer (wavenet.py:351), the skip weights unless the first of several groups took them, the last grouped launch.
        (Base layer as a TN GEMM over a materialised one-hot matrix: 0.044 ms + 29 MB written by base_gather.  The
        scatter-add form - rows of dx0 added into LDS images per 64 channels, AEW-internal experiment of round 2 - took
        0.58 ms: the rows have to be fetched one dependent (wav[t] -> dx0[t]) load pair at a time and the partial images
        merged with ~10 M global atomics; the GEMM streams the same bytes at full rate)"""
        p = self.pre
        # (the gradient is [Rp][Qp]; the packed form is the transposed fp32 gather table [Q][Rp]: no shared layout)
        rt.add("base", self._tn(self.T, self.R, self.Rp, dx0.seg(self.Rp), [self.onehot.seg(self.Qp)]), TAG_MISC, rt.LAST,
               bias=(p + "base_layer.bias", dx0, "db.base"),
               pieces=[Piece(p + "base_layer.weight", 0, [self.Q, 1], [self.R, self.Q], 0, [self.Qp, 1])])
        rt.merge_early()
        if not rt.multi:
            self._bwd_skip_wgrad(rt)
        rt.emit_last(tail, join=n_chains > 1)

    def _bwd_spk(self, plan: Plan, rt: "WgradRouter", colsum_tbl: CopyTableBuilder, tail: int):
        """Speaker / gated-bias gradients (of the layers the first of several groups has not done already)."""
        running = max(0, self.NL - self.wgrad_split_layers) if rt.grouped else 0
        sb = self._spk_bwd(0, self.hi_first_layer or 0, running, "lo")
        with plan.side(tail or 1):                                 # reads the side lanes' wgrad slabs: side join
            colsum_tbl.emit(plan, "colsum.dfg (from wgrad column R)", join=True)
            plan.add(L.OP_SPK_BWD, sb, "spk_bwd", TAG_MISC, join=not colsum_tbl.recs)

    def _bwd_cond(self, plan: Plan, n_chains: int):
        """Conditioning gradient over all layers' dfg (wavenet.py:100-101 cond terms).  With split_multiseg the layers
        [n_lo, NL) were summed on a side lane mid-chain (dcond_part); this GEMM adds them."""
        g, Dp, Cp, half = self.g, self.Dp, self.Cp, self.n_lo < self.NL
        segs = [self.dfg[l].seg(2 * Dp, row_off=-g.layers[l].cond_lead) for l in range(self.n_lo)]
        plan.add(L.OP_GEMM_NT, make_nt(BF, self.T, Cp, Cp, self.B, segs, self.VfgT_lo.ptr, flags=L.EF_ADD_AUX0 if half else 0,
                                       out0=self.dcond.view(), aux0=self.dcond_part.view() if half else None,
                                       impl=self.impl if half else self._impl("dcond")), "dcond", TAG_DCOND,
                 # (two chains: the main lane meets them here at the latest, in every lane mode)
                 join=("lane", self.EARLY_LANE) if half else n_chains > 1)

    def _bwd_ups(self, plan: Plan, rt: "WgradRouter"):
        """Upsamplers, last stage first (wavenet.py:154), LC conv (wavenet.py:337) and the jitter scatter."""
        B, g, hps, p, ps, impl = self.B, self.g, self.hps, self.pre, self.ps, self.impl
        Clc, Cp, Lp = self.Clc, self.Cp, self.Lp
        n_ups = len(hps.lc_upsample_strides)
        for i in range(n_ups - 1, -1, -1):
            f, s = hps.lc_upsample_filt_sizes[i], hps.lc_upsample_strides[i]
            X, dX = self.ups_in[i], self.dups[i]
            last = i == n_ups - 1
            dY = self.dcond if last else self.dups[i + 1]
            trim0 = g.trim_ups_out[0] if last else 0
            self._colsum(plan, dY, dY.rows, Clc, ps.ptr(p + f"lc_upsample.{i}.tconv.bias", True), label=f"db.up{i}")
            segs = [dY.seg(Cp, row_step=s, row_off=k - (f - s) - trim0) for k in range(f)]
            rt.add(f"up{i}", self._tn(X.rows, Clc, Cp, X.seg(Cp), segs), TAG_UPS, rt.UPS)
            plan.add(L.OP_GEMM_NT, make_nt(BF, X.rows, Cp, Cp, B, segs, self.WupT[i].ptr, out0=dX.view(),
                                           impl=impl), f"d.ups{i}", TAG_UPS)
        dlc1, lc1 = self.dups[0], self.ups_in[0]
        rt.add("lc", self._tn(lc1.rows, Clc, Cp, dlc1.seg(Cp), [self.lcj.seg(Lp, row_off=t) for t in range(3)]),
               TAG_UPS, rt.UPS, bias=(p + "lc_conv.bias", dlc1, "db.lc"))
        rt.emit_ups()
        plan.add(L.OP_GEMM_NT, make_nt(BF, self.Ne, ru(self.n_lc_in, 8), Lp, B, [dlc1.seg(Cp, row_off=-t) for t in range(3)],
                                       self.WlcT.ptr, out0=self.dlcj.view(), impl=impl), "d.lc_conv", TAG_UPS)
        # ---- jitter scatter back to the LC source
        if L.load().aew_lc_scatter_needs_zero(self.Ne):            # (short windows: the scatter runs in its gather form, which
            plan.zero(self.ws, self.dlc_src.name)                  #  writes every element: no atomics, no zeroing)
        sc = L.LcScatter()
        sc.d, sc.d_bs, sc.d_pitch = self.dlcj.ptr, self.dlcj.bs, self.dlcj.pitch
        sc.jitter, sc.jit_pitch = self.jitter.data_ptr(), self.jitter.shape[1]
        sc.dsrc, sc.dsrc_bs, sc.dsrc_pitch = self.dlc_src.ptr, self.dlc_src.bs, self.dlc_src.pitch
        sc.B, sc.N, sc.C, sc.take_compat = B, self.Ne, self.n_lc_in, int(self.take_compat)
        plan.add(L.OP_LC_SCATTER, sc, "lc_scatter", TAG_UPS)


class WgradRouter:
    """Where each weight gradient of one decoder backward plan runs, and which table unpacks it.
    Destinations: its own split-K TN op on the next rotating side lane (wgrad_group 0, the check kernels, the top
    wgrad_split_layers layers); the current grouped launch (AEW_OP_GEMM_TN_GROUP; impl 0 only) of wgrad_group layers,
    emitted on a side lane right after the dz GEMM of its lowest layer; the last grouped launch, after the chain; the
    upsampler group, where long contractions are cut into row chunks.
    Several groups (wgrad_group < NL; data parallel: AEW_WGRAD_GROUP = NL / 2): the post-network and skip weight gradients -
    operands complete before the chain starts - join the FIRST group instead of the last and are unpacked with it.  Every
    gradient from layer NL - wgrad_group up (the tail of the flat buffer, `hi_first_layer`) is then final right after
    "unpack grads (decoder, upper layers)": a data-parallel caller starts its reduce-scatter there, under the second half
    of the chain (TrainEngine.bwd_a1 / bwd_a2).
    Tables: what is final mid-chain goes to the early table - emitted after the first of several groups or, ungrouped,
    after layer NL // 2 - the rest to the packer's own, which also takes the early records of a single group."""
    LATE, LAST, UPS = -1, -2, -3      # placements other than a layer index: operands exist early, the result is needed at the
                                      # end | needs dx of layer 0: last group | upsampler / LC-conv group

    def __init__(self, dec: DecoderPlan, plan: Plan, early_tbl: Optional[CopyTableBuilder]):
        self.dec, self.plan = dec, plan
        self.grouped = dec.wgrad_group > 0 and dec.impl == 0
        self.multi = self.grouped and dec.wgrad_group < dec.NL
        if self.multi and dec.wgrad_split_layers > 0:
            # (the upper-layers spk_bwd differences RUNNING column sums; layers kept as split-K ops deliver per-batch sums)
            raise ValueError("wgrad_split_layers > 0 cannot be combined with several grouped weight-gradient launches (wgrad_group < layers)")
        self.late = dec.pk.unpack_tbl
        self.early = early_tbl                                 # until it is emitted or merged
        self.tbl = self.late if early_tbl is None else early_tbl      # table of a result that is final now
        self.grp: Optional[TnGroupBuilder] = None
        self.n_groups = self.layers_in_grp = 0
        self.tail: List[Tuple[L.GemmTN, str]] = []             # (descriptor, label): join the last group
        self.ups = TnGroupBuilder(dec.ws, dec.pre + "tng_ups", 128) if self.grouped else None

    def in_group(self, l: int) -> bool:
        """Layer l's weight gradients go to a grouped launch (which then also delivers its running column sums of dfg)."""
        return self.grouped and l < self.dec.NL - self.dec.wgrad_split_layers

    def _group(self) -> TnGroupBuilder:
        dec = self.dec
        if self.grp is None:
            n128 = dec.NL * ((2 * dec.Dp // 128) * ((2 * dec.Rp + dec.Cp) // 128) + (dec.Rp // 128) * (dec.Dp // 128))   # (wgrad_tile)
            tile = dec.wgrad_tile or (256 if n128 > TnGroupBuilder.CURSOR_AUTO_TILES else 128)
            self.grp = TnGroupBuilder(dec.ws, dec.pre + f"tng{self.n_groups}", tile)
            self.grp.cursor = dec.wgrad_cursor
        return self.grp

    def add(self, name: str, t: "L.GemmTN", tag: int, place: int, bias: Optional[Tuple[str, Mat, str]] = None,
            pieces: Optional[Sequence[Piece]] = None) -> WGrad:
        """Routes descriptor t (place: layer index | LATE | LAST | UPS), allocates `<pre>wg.<name>`, points t at it and
        writes the unpack records (pieces: the result's index map; default: the packed matrix's, DecoderPlan.lay[name]).
        bias = (bias parameter, G operand, label): the bias gradient is the column sums of the G operand - a by-product
        of a grouped descriptor, a column-sum op where there is no block that sees every row (split-K, row-split)."""
        dec = self.dec
        if not self.grouped:
            dest = None
        elif place == self.UPS:
            dest = self.ups
        elif place >= 0:
            dest = self._group() if self.in_group(place) else None
        else:
            dest = self._group() if (self.multi and place == self.LATE) else self.tail
        # upsampler group: one or a few output tiles with up to 8 x 1780 rows to contract, cut into chunks of ~512 rows
        # (one block and one slab each) unless the whole contraction is that short
        split = dest is self.ups and dest is not None and t.Mc * t.batch > dec.ups_split_rows
        bias_ptr = dec.ps.ptr(bias[0], True) if (bias and dec.ps.has(bias[0])) else 0
        if dest is None or split:
            if bias_ptr:
                dec._colsum(self.plan, bias[1], t.Mc, t.N, bias_ptr, label=bias[2])
        else:
            t.colsum_out = bias_ptr or None
        slabs = L.tn_slabs(t) if dest is None else (dest.set_split(t, 512) if split else 1)
        g = wgrad_slab(dec.ws, dec.pre + "wg." + name, t, slabs, self.late if dest is self.tail else self.tbl)
        dec.pk.unpack(dec.lay[name] if pieces is None else pieces, g)
        if dest is None:
            with self.plan.side(dec._next_lane()):             # off the dgrad chain
                self.plan.add(L.OP_GEMM_TN, t, "wgrad." + name, tag)
        elif dest is self.tail:
            self.tail.append((t, "wgrad." + name))
        else:
            dest.add(t, "wgrad." + name)
        return g

    def _unpack_early(self):
        with self.plan.side(1):                                # after the wgrads issued so far, on any lane
            self.early.emit(self.plan, "unpack grads (decoder, upper layers)", join=True)
        self.early, self.tbl = None, self.late

    def layer_done(self, l: int):
        """After layer l's weight gradients: a group that holds wgrad_group layers is emitted (never at layer 0: what is
        left goes with the last group), and the first one is followed by the early unpack."""
        dec, plan = self.dec, self.plan
        self.layers_in_grp += self.in_group(l)
        if self.grp is None or self.layers_in_grp < dec.wgrad_group or l == 0:
            return
        self.layers_in_grp = 0
        with plan.side(dec._next_lane()):
            self.grp.emit(plan, f"wgrad.group{self.n_groups} (layers {l}.., skip, post)" if self.n_groups == 0 else
                          f"wgrad.group{self.n_groups} (layers {l}..)", TAG_WG_FG)
        self.grp, self.n_groups = None, self.n_groups + 1
        if self.early is not None:
            # gated-bias / speaker-projection gradients of the layers in this group (from the running column sums it just
            # wrote): everything of layers >= l = NL - wgrad_group is final after the unpack below
            dec.hi_first_layer = l
            sb = dec._spk_bwd(l, dec.NL - l, dec.NL, "hi")
            with plan.side(1):
                plan.add(L.OP_SPK_BWD, sb, "spk_bwd (upper layers)", TAG_MISC, join=True)
            self._unpack_early()

    def dx_done(self, l: int):
        """After dx of layer l: the ungrouped plan unpacks the upper half's gradients here; after the chain nothing is early."""
        if not self.grouped and self.early is not None and l == self.dec.NL // 2:
            self._unpack_early()
        if l == 0:
            self.tbl = self.late

    def merge_early(self):
        """A plan that unpacked nothing mid-chain (a single group): its early records join the packer's table here."""
        if self.early is not None:
            self.late.recs.extend(self.early.recs)
            self.early = None

    def emit_last(self, lane: int, join: bool):
        """The last grouped launch: the layers left, and what was deferred to it."""
        if not self.grouped:
            return
        for t, label in self.tail:
            self._group().add(t, label)
        with self.plan.side(lane or self.dec._next_lane()):
            self.grp.emit(self.plan, f"wgrad.group{self.n_groups} (last layers, skip, post)" if not self.multi else
                          f"wgrad.group{self.n_groups} (layers 0.., base)", TAG_WG_FG, join=join)
        self.grp = None

    def emit_ups(self):
        if self.ups is not None:
            with self.plan.side(self.dec._next_lane()):
                self.ups.emit(self.plan, "wgrad.group (upsamplers, lc conv)", TAG_UPS)


# ------------------------------------------------------------------------------------------
# encoder + bottleneck (fp32 exact chain)
# ------------------------------------------------------------------------------------------
def det_colsum(ws: Workspace, cs: "L.Colsum", name: str):
    """Scratch + tickets of the deterministic form of a column-sum op (aew_colsum_t.det_scratch / det_tickets: partial sums per
    row chunk, added in a fixed order by the last arriver - no fp32 atomics).  The tickets start at zero and every launch
    leaves them at zero."""
    nf, nt = C.c_int64(0), C.c_int32(0)
    L.check(L.load().aew_colsum_det_size(C.byref(cs), C.byref(nf), C.byref(nt)), "aew_colsum_det_size")
    cs.det_scratch = ws.alloc(name + ".scratch", max(4, nf.value), torch.float32).data_ptr()
    cs.det_tickets = ws.alloc(name + ".tickets", max(4, nt.value), torch.int32, zero=True).data_ptr()


def colsum_op(ws: Workspace, x: "L.Seg", dtype: int, M: int, N: int, batch: int, out_ptr: int, out_bs: int, det: str) -> "L.Colsum":
    """Column sums of x [batch][M][N] added into out (pre-zeroed by the plan), deterministic (det_colsum, buffers `det`.*)."""
    cs = L.Colsum()
    cs.x, cs.dtype, cs.M, cs.N, cs.batch = x, dtype, M, N, batch
    cs.out, cs.out_bs, cs.accumulate = out_ptr, out_bs, 1
    det_colsum(ws, cs, det)
    return cs


def exact_split_args(ws: Workspace, name: str, S: int, cin: int, k_total: int, rows: int, n_pad: int) -> dict:
    """make_nt keywords for the split-K form of an exact fp32 GEMM (aew_gemm_nt_t.k_split): S contiguous k-ranges on
    separate workgroups, combined in a fixed order - the canonical summation order of the op, oracle/exact.py ksplit_for
    states the same rule: the input channels need no padding (cin a multiple of 64) and the K axis is a multiple of 32 * S.
    Allocates the partial-sum slabs and the (self-resetting) tickets.  {} = not split."""
    if S not in (2, 4) or cin % 64 or k_total % (32 * S):
        return {}
    rows_pad = ru(rows, 32)
    wsb = ws.alloc(name + ".ws", S * rows_pad * n_pad, torch.float32)
    tk = ws.alloc(name + ".tickets", (rows_pad // 16) * (n_pad // 64) * 4, torch.int32)
    return dict(k_split=S, ksplit_ws_ptr=wsb.data_ptr(), ksplit_tickets_ptr=tk.data_ptr())


class EncoderPlan:
    """Encoder (wave_encoder.py:34-103).  Forward: fp32, exact k-ascending chains (bit-exact code indices against
    oracle/exact_chain.c).  Backward: bf16 operands, fp32 accumulation on the bf16 MFMA kernels - the forward's
    exactness contract does not extend to gradients, and the fp32 kernels spent 0.48 ms per step here (9.5 % of the
    step for 0.3 % of its FLOPs: one serial chain per output, every 16-row tile re-streaming the weight matrix).  The
    forward's epilogue writes what the backward reads as bf16: the activations (wgrad operand), the pre-activation
    (relu mask)."""

    k_split = 0               # 2 | 4: the exact fp32 GEMMs (encoder layers, bottleneck linear) as S contiguous k-ranges on separate
                              # workgroups with a fixed-order combine (aew_gemm_nt_t.k_split) - a DIFFERENT canonical summation
                              # order, which oracle/exact.py's KSPLIT must then state too (the GPU test sets both).  Built for
                              # the round-4 review's item 5 and measured: enc.# 0.266 ms unsplit, 0.291 ms with S = 4 (720
                              # workgroups instead of 180: the serial K loop per workgroup is a quarter, the launch is not
                              # faster - these layers are bound by what a workgroup streams per K tile, profiles/r04_notes.md
                              # 9), fwd_a 0.379 / 0.370 / 0.387 ms for S = 0 / 2 / 4.  Off: the order stays one chain per output

    def __init__(self, ws: Workspace, ps: ParamStore, hps, geom: G.ModelGeom, B: int, n_mel: int,
                 mel_cl: Mat, packer: Packer, impl: int = 0, in_tbl: Optional[CopyTableBuilder] = None,
                 in_mel: Optional[torch.Tensor] = None, wgrad_group: Optional[int] = None):
        self.ws, self.ps, self.hps, self.g, self.B, self.impl = ws, ps, hps, geom, B, impl
        self.wgrad_group = DecoderPlan.wgrad_group if wgrad_group is None else int(wgrad_group)
        self.pk = packer
        self.n_mel, self.Mp, self.Mb = n_mel, ru(n_mel, 64), ru(n_mel, 128)
        self.E, self.Ep, self.Eb = hps.enc_n_out, ru(hps.enc_n_out, 64), ru(hps.enc_n_out, 128)
        self.lens = geom.enc_lens                      # 10 entries
        E, Ep, Eb = self.E, self.Ep, self.Eb
        self.y: List[Mat] = [mel_cl]                   # fp32 activations (forward chain)
        self.yb: List[Mat] = [Mat.new(ws, "enc.yb0", B, self.lens[0], self.Mb, BF)]    # bf16 copies (wgrad operand)
        if in_tbl is not None and in_mel is not None:
            in_tbl.add(in_mel.data_ptr(), self.yb[0].ptr, [B, geom.mel_len, n_mel], [n_mel * geom.mel_len, 1, geom.mel_len],
                       [self.yb[0].bs, self.Mb, 1], F3, BF)
        self.r: List[Optional[Mat]] = [None]           # bf16 pre-activations (relu mask of the backward)
        for i in range(9):
            self.y.append(Mat.new(ws, f"enc.y{i + 1}", B, self.lens[i + 1], Ep, F3))
            self.yb.append(Mat.new(ws, f"enc.yb{i + 1}", B, self.lens[i + 1], Eb, BF))
            self.r.append(Mat.new(ws, f"enc.r{i + 1}", B, self.lens[i + 1], Eb, BF))
        self.dy = [Mat.new(ws, f"enc.dy{i}", B, self.lens[i], self.Mb if i == 0 else Eb, BF) for i in range(10)]
        self.dpre = [None] + [Mat.new(ws, f"enc.dpre{i}", B, self.lens[i], Eb, BF) for i in range(1, 10)]
        self.zero_cnt = ws.alloc("enc.zero_cnt", 9, torch.int64)
        self.W, self.WT, self.bias = [], [], []
        cin, cinp, cinb = n_mel, self.Mp, self.Mb
        for i, (f, s) in enumerate(zip(G.ENCODER_FILTERS, G.ENCODER_STRIDES)):
            nm = f"encoder.net.{i}.conv."
            Wm = Mat.new(ws, f"enc.wp.{i}", 1, Ep, f * cinp, F3)
            packer.pack(self._w_piece(i, cinp), Wm, first=(i == 0))
            self.W.append(Wm)
            # dgrad layouts, bf16, per output phase ph < s: [ci][j*Eb + co] <- W[co][ci][ph + s*j]
            phs = []
            for ph in range(s):
                WT = Mat.new(ws, f"enc.wpT.{i}" + (f".{ph}" if s > 1 else ""), 1, cinb, (f // s) * Eb, BF)
                packer.pack(Piece(nm + "weight", ph, [cin * f, f, s], [E, cin, f // s], 0, [1, (f // s) * Eb, Eb]), WT, late=True)
                phs.append(WT)
            self.WT.append(phs)
            bt = ws.alloc(f"enc.wp.bias{i}", Ep, torch.float32)
            (packer.first_tbl if (i == 0 and packer.first_tbl is not None) else packer.pack_tbl).add(
                ps.ptr(nm + "bias"), bt.data_ptr(), [E], [1], [1], F3, F3)
            self.bias.append(bt)
            cin, cinp, cinb = E, Ep, Eb

    def _w_piece(self, i: int, pitch: int) -> Piece:
        """Layer i's conv weight [E][cin][f] as [E][f * pitch], tap-major with the input channels padded to `pitch`: the
        forward's fp32 matrix (pitch = channels rounded up to 64) and the weight gradient (to 128, the bf16 operand's)."""
        cin, f = (self.n_mel if i == 0 else self.E), G.ENCODER_FILTERS[i]
        return Piece(f"encoder.net.{i}.conv.weight", 0, [cin * f, f, 1], [self.E, cin, f], 0, [f * pitch, 1, pitch])

    def build_forward(self, plan: Plan, join_before_layer1=False):
        """join_before_layer1: join spec (see Plan.add) for the layer-1 GEMM - the side lane that packs the weights of
        layers 1.. while layer 0 (whose own weights were packed on the main lane) runs."""
        B, impl, Ep = self.B, self.impl, self.Ep
        plan.zero(self.ws, "enc.zero_cnt")
        cinp = self.Mp
        for i, (f, s, res) in enumerate(zip(G.ENCODER_FILTERS, G.ENCODER_STRIDES, G.ENCODER_RESIDUAL)):
            X, Y, Rm = self.y[i], self.y[i + 1], self.r[i + 1]
            segs = [X.seg(cinp, row_step=s, row_off=k) for k in range(f)]
            flags = L.EF_BIAS | L.EF_RELU | L.EF_OUT1_PRE | L.EF_COUNT_ZERO | L.EF_OUT2_COPY | (L.EF_ADD_AUX0 if res else 0)
            cin = self.n_mel if i == 0 else self.E
            skw = exact_split_args(self.ws, f"enc.ks{i}", self.k_split if impl == 0 else 0, cin, f * cinp, Y.rows * B, Ep)
            plan.add(L.OP_GEMM_NT, make_nt(
                F3, Y.rows, self.E, Ep, B, segs, self.W[i].ptr, flags=flags, out0=Y.view(), out1=Rm.view(),
                out2=self.yb[i + 1].view(),
                aux0=X.view(row_off=(f - 1) // 2) if res else null_view(), bias_ptr=self.bias[i].data_ptr(),
                counter_ptr=self.zero_cnt.data_ptr() + 8 * i, impl=impl, **skw), f"enc.{i}", TAG_ENC,
                join=join_before_layer1 if i == 1 else False)
            cinp = Ep

    def build_backward(self, plan: Plan, need_input_grad: bool = True):
        """Expects dy[9] and dpre[9] already written (by the bottleneck backward)."""
        B, impl, E, Eb, ps, pk = self.B, self.impl, self.E, self.Eb, self.ps, self.pk
        # grouped mode (DecoderPlan.wgrad_group): the nine weight gradients as ONE launch after the dgrad chain (each
        # contracts over 8 x 29..70 rows: nine launches of a few microseconds of work each otherwise), the bias
        # gradients as its column-sum by-product
        grp = TnGroupBuilder(self.ws, "enc.tng", 128) if (self.wgrad_group > 0 and impl == 0) else None
        for i in range(8, -1, -1):
            f, s, res = G.ENCODER_FILTERS[i], G.ENCODER_STRIDES[i], G.ENCODER_RESIDUAL[i]
            X = self.yb[i]
            cin, cinb = (self.n_mel, self.Mb) if i == 0 else (E, Eb)
            dpre, dyo = self.dpre[i + 1], self.dy[i + 1]
            Lo = dpre.rows
            t = make_tn(BF, Lo, B, E, Eb, dpre.seg(Eb), [X.seg(cinb, row_step=s, row_off=k) for k in range(f)],
                        impl=impl)
            if grp is None:
                cs = colsum_op(self.ws, dpre.seg(128), BF, Lo, E, B, ps.ptr(f"encoder.net.{i}.conv.bias", True), 0, f"det.db.enc{i}")
                with plan.side(1 + (2 * i) % DecoderPlan.n_side_lanes):
                    plan.add(L.OP_COLSUM, cs, f"db.enc{i}", TAG_ENC)
            wg = wgrad_slab(self.ws, f"enc.wg.{i}", t, L.tn_slabs(t) if grp is None else 1, pk.unpack_tbl)
            if grp is None:
                with plan.side(1 + (2 * i + 1) % DecoderPlan.n_side_lanes):
                    plan.add(L.OP_GEMM_TN, t, f"wgrad.enc{i}", TAG_ENC)
            else:
                t.colsum_out = ps.ptr(f"encoder.net.{i}.conv.bias", True)
                grp.add(t, f"wgrad.enc{i}")
            pk.unpack([self._w_piece(i, cinb)], wg)
            if i == 0 and not need_input_grad:
                continue
            dX = self.dy[i]
            Li = dX.rows
            lw = (f - 1) // 2
            for ph in range(s):
                Mq = (Li - ph + s - 1) // s
                if Mq <= 0:
                    continue
                segs = [dpre.seg(Eb, row_off=-j) for j in range(f // s)] if s > 1 else \
                       [dpre.seg(Eb, row_off=-k) for k in range(f)]
                flags = (L.EF_ADD_AUX0 if res else 0) | (L.EF_OUT1_POS1 if i > 0 else 0)
                plan.add(L.OP_GEMM_NT, make_nt(
                    BF, Mq, ru(cin, 8), cinb, B, segs, self.WT[i][ph].ptr, flags=flags,
                    out0=dX.view(row_step=s, row_off=ph),
                    out1=self.dpre[i].view(row_step=s, row_off=ph) if i > 0 else null_view(),
                    aux0=dyo.view(row_step=s, row_off=ph - lw) if res else null_view(),
                    aux1=self.r[i].view(row_step=s, row_off=ph) if i > 0 else null_view(), impl=impl),
                    f"d.enc{i}.ph{ph}", TAG_ENC)
        if grp is not None:
            with plan.side(1):
                grp.emit(plan, "wgrad.group (encoder)", TAG_ENC)


# ------------------------------------------------------------------------------------------
# bottleneck (fp32): the shared linear + one subclass per type
# ------------------------------------------------------------------------------------------
def reduce_op(terms: Sequence[Tuple[int, int, float]], out_ptr: int) -> "L.Reduce":
    """out[0] = sum_i scale_i * sum(x_i[:n_i]), out[1 + i] = term i (aew_reduce_t) over terms [(x_ptr, n, scale), ...]."""
    red = L.Reduce()
    red.n_terms = len(terms)
    for i, (p_, n_, s_) in enumerate(terms):
        red.x[i], red.n[i], red.scale[i], red.post_scale[i] = p_, n_, s_, 1.0
    red.out = out_ptr
    return red


class BottleneckPlan:
    """Bottleneck between the encoder and the decoder's conditioning input.  This class owns what every type shares: the
    linear (bn.lin = y9 @ Wl^T, its packed weights, its weight / data gradient).  A subclass per type states, each once:
    its buffers (_alloc), its ops in fwd_a / fwd_b (_forward, build_diag), its loss and metric terms, its nll scale, its
    backward op (_backward), its part of the module surface's metric map (metrics) and - vqvae-ema - the codebook plan
    (build_codebook) and the restart op.  make() is the one place that reads the type string.  The mfcc inverter has no bottleneck."""

    K = 0                     # codes; the evaluation accumulates code statistics iff K > 0 (then ind / min_dist are buffers)
    ind = min_dist = None
    eps = None                # vae: the noise the caller supplies (TrainEngine.set_inputs)
    lin_outs = 1              # outputs of the linear per code dimension
    lin_flags, lin_bias_ptr = 0, 0      # epilogue flags and bias of the bn.linear op
    names = ("d", "dp", "Q", "nlin_p", "lin", "code")     # what TrainEngine republishes as its own attributes

    @staticmethod
    def make(bn_type: str, *args, **kw) -> "BottleneckPlan":
        types = {"vqvae-ema": VqEmaBottleneck, "vqvae": VqBottleneck, "vae": VaeBottleneck, "ae": AeBottleneck}
        if bn_type not in types:
            raise ValueError(f"unknown bn_type {bn_type}")
        return types[bn_type](*args, **kw)

    def __init__(self, ws: Workspace, ps: ParamStore, hps, geom: G.ModelGeom, B: int, enc: "EncoderPlan", packer: Packer,
                 impl: int = 0, loss_mode: str = "intended"):
        self.ws, self.ps, self.hps, self.g, self.B, self.enc, self.pk, self.impl = ws, ps, hps, geom, B, enc, packer, impl
        E, d, Ne = hps.enc_n_out, hps.bn_n_out, geom.embed_len
        self.loss_mode, self.E, self.Ep = loss_mode, E, ru(E, 64)
        self.d, self.dp, self.Q, Ep = d, ru(d, 64), B * Ne, self.Ep
        self.nlin = nlin = self.lin_outs * d
        self.nlin_p = ru(nlin, 64)
        self.lin = Mat.new(ws, "bn.lin", B, Ne, self.nlin_p, F3)          # ze / (mu|logvar)
        self.Wl = Mat.new(ws, "bn.wp.lin", 1, self.nlin_p, Ep, F3)
        self.WlT = Mat.new(ws, "bn.wp.linT", 1, Ep, self.nlin_p, F3)
        self.lin_piece = Piece("bottleneck.linear.weight", 0, [E, 1], [nlin, E], 0, [Ep, 1])     # Wl, and its gradient
        packer.pack(self.lin_piece, self.Wl)
        packer.pack(self.lin_piece.at(0, [1, self.nlin_p]), self.WlT)
        self.dlin = Mat.new(ws, "bn.dlin", B, Ne, self.nlin_p, F3)
        # words of the engine that the ops read: the loss record, the upstream gradient, the chained launches' sticky guard
        self.loss_ptr, self.gmul_ptr, self.guard_ptr = ws.ptr("loss"), ws.ptr("loss.gmul"), ws.ptr("chain.guard")
        self._alloc()

    # -- forward --------------------------------------------------------------------------
    def build_forward(self, fa: Plan, fb: Plan):
        """bn.linear and the type's ops behind it into fwd_a; side work that only the next step reads into fwd_b."""
        B, Ne, Ep, impl = self.B, self.g.embed_len, self.Ep, self.impl
        skw = exact_split_args(self.ws, "bn.ks", EncoderPlan.k_split if impl == 0 else 0, self.E, Ep, Ne * B, self.nlin_p)
        fa.add(L.OP_GEMM_NT, make_nt(F3, Ne, ru(self.nlin, 4), self.nlin_p, B, [self.enc.y[9].seg(Ep)],
                                     self.Wl.ptr, flags=self.lin_flags, out0=self.lin.view(),
                                     bias_ptr=self.lin_bias_ptr, impl=impl, **skw),
               "bn.linear", TAG_VQ)
        self._forward(fa, fb)

    def build_diag(self, fb: Plan, lane: int, w: int, scratch: torch.Tensor, out: torch.Tensor):
        """Codebook / encoder-output statistics (vqema_bn.py:254-260) on a side lane of fwd_b: the VQ types."""

    def metric_terms(self) -> List[Tuple[int, int, float]]:
        """Terms of the forward's metrics reduction behind rec and tprb_m."""
        return []

    def loss_op(self, nll: Tuple[int, int, float]) -> "L.Reduce":
        """The loss reduction: `nll` is the decoder's term (pointer, count, mean or sum scale: model.MEAN_LOSS)."""
        return reduce_op(self.loss_terms(nll), self.loss_ptr)

    def nll_scale(self, scale: float) -> float:
        """The factor at which the NLL gradient enters the backward, given the loss's mean / sum scale."""
        return scale

    def metrics(self, met: torch.Tensor, diag: torch.Tensor, loss: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The type's part of objective.metrics: name -> view of the metrics / diagnostics / loss records."""
        return {}

    # -- backward -------------------------------------------------------------------------
    def build_backward(self, bw: Plan, dcode: Mat):
        """d(loss)/d(code) [B][Ne][dp] -> dlin (the type's op), then the linear's weight and data gradient; leaves dy[9] and
        dpre[9] of the encoder written."""
        B, Ne, Ep, impl, enc = self.B, self.g.embed_len, self.Ep, self.impl, self.enc
        self._backward(bw, dcode)
        t = make_tn(F3, Ne, B, self.nlin, self.nlin_p, self.dlin.seg(64), [enc.y[9].seg(Ep)], impl=impl)
        wg = wgrad_slab(self.ws, "bn.wg.lin", t, L.tn_slabs(t), self.pk.unpack_tbl)
        with bw.side():
            bw.add(L.OP_GEMM_TN, t, "wgrad.bn.linear", TAG_VQ)
        self.pk.unpack([self.lin_piece], wg)
        bw.add(L.OP_GEMM_NT, make_nt(F3, Ne, self.E, Ep, B, [self.dlin.seg(self.nlin_p)],
                                     self.WlT.ptr, flags=L.EF_OUT1_POS1, out0=enc.dy[9].view(),
                                     out1=enc.dpre[9].view(), aux1=enc.r[9].view(), impl=impl),
               "d.bn.linear", TAG_VQ)

    def build_codebook(self):
        """vqvae-ema: the plan `cb` that refreshes the codebook after the backward."""


class VqBottleneck(BottleneckPlan):
    """vq_bn.py:28-61, 72-115: the codebook is a parameter; the loss sums NLL + (1 + gamma) * ||ze - emb[ind]||^2."""
    metric = 1                # aew_vq_nearest_t.metric / aew_vq_bwd_t.metric
    names = BottleneckPlan.names + ("K", "ind", "min_dist", "emb")

    def _alloc(self):
        ws, B, Ne = self.ws, self.B, self.g.embed_len
        self.K = self.hps.bn_vq_n_embed
        self.code = Mat.new(ws, "bn.zq", B, Ne, self.dp, F3)
        self.ind = ws.alloc("bn.ind", self.Q, torch.int64)
        self.min_dist = ws.alloc("bn.min_dist", self.Q, torch.float32)
        self._alloc_codebook()

    def _alloc_codebook(self):
        self.emb, self.demb_ptr = self.ps.view("bottleneck.emb"), self.ps.ptr("bottleneck.emb", True)

    def _forward(self, fa: Plan, fb: Plan):
        vq = L.VqNearest()
        vq.ze, vq.emb = self.lin.ptr, self.emb.data_ptr()
        vq.Q, vq.K, vq.d, vq.d_pitch = self.Q, self.K, self.d, self.nlin_p
        vq.metric = self.metric
        vq.ind, vq.dist, vq.zq = self.ind.data_ptr(), self.min_dist.data_ptr(), self.code.ptr
        vq.n_split = max(1, min(16, self.K // 256))       # each block scans >= 256 codes (one per thread)
        if vq.n_split > 1:
            vq.scratch = self.ws.alloc("bn.vq_part", 2 * self.Q * vq.n_split, torch.float32).data_ptr()
        assert self.dp == self.nlin_p
        fa.add(L.OP_VQ_NEAREST, vq, "vq.nearest", TAG_VQ)

    def lookup_op(self, bad: torch.Tensor) -> "L.CodeLookup":
        """The inverse of vq.nearest on its zq output: bn.zq from the codes in bn.ind (aew_code_lookup_t), same layouts;
        `bad` takes the number of codes outside [0, K)."""
        lk = L.CodeLookup()
        lk.ind, lk.emb, lk.zq, lk.bad = self.ind.data_ptr(), self.emb.data_ptr(), self.code.ptr, bad.data_ptr()
        lk.Q, lk.K, lk.d, lk.d_pitch = self.Q, self.K, self.d, self.nlin_p
        return lk

    def _diag_op(self, w: int, scratch: torch.Tensor, out: torch.Tensor) -> "L.VqDiag":
        dv = L.VqDiag()
        dv.ze, dv.Q, dv.d, dv.d_pitch = self.lin.ptr, self.Q, self.d, self.lin.pitch
        dv.K, dv.emb = self.K, self.emb.data_ptr()
        dv.B, dv.w, dv.n_quant = self.B, w, self.hps.n_quant
        dv.scratch, dv.out = scratch.data_ptr(), out.data_ptr()
        return dv

    def build_diag(self, fb, lane, w, scratch, out):
        with fb.side(lane):
            fb.add(L.OP_VQ_DIAG, self._diag_op(w, scratch, out), "diagnostics (codebook)", TAG_LOSS)

    def metric_terms(self):
        return [(self.min_dist.data_ptr(), self.Q, float(self.hps.bn_vq_gamma) / self.Q)]              # com

    def loss_terms(self, nll):
        return [nll, (self.min_dist.data_ptr(), self.Q, 1.0 + float(self.hps.bn_vq_gamma))]

    def metrics(self, met, diag, loss):
        m = {"com": met[3], "min_ze": diag[0], "max_ze": diag[1], "min_emb": diag[2], "max_emb": diag[3]}   # vqema_bn.py:254-257
        m.update(self._usage_metrics(diag))
        return m

    def _usage_metrics(self, diag):
        return {"nunq": self.ind[:self.Q].unique().numel()}

    def _backward(self, bw: Plan, dcode: Mat):
        vb = L.VqBwd()
        vb.ze, vb.emb, vb.ind, vb.dzq = self.lin.ptr, self.emb.data_ptr(), self.ind.data_ptr(), dcode.ptr
        vb.Q, vb.d, vb.d_pitch = self.Q, self.d, self.nlin_p
        vb.metric = self.metric
        vb.coef = float(self.hps.bn_vq_gamma)
        vb.demb_coef = 1.0
        vb.dze = self.dlin.ptr
        vb.demb = self.demb_ptr
        vb.gmul = self.gmul_ptr
        bw.add(L.OP_VQ_BWD, vb, "vq.bwd", TAG_VQ)


class VqEmaBottleneck(VqBottleneck):
    """vqema_bn.py:125-222, 231-266: the codebook follows exponential averages of the encoder outputs assigned to each
    code; the loss sums NLL + gamma * commitment (loss_mode "head": the commitment alone, vqema_bn.py:246)."""
    metric = 0
    names = VqBottleneck.names + ("ema_numer", "ema_denom", "zn_sum", "z_sum", "n_sum", "ind_hist", "n_sum_diag", "cb")

    def _alloc_codebook(self):
        ws, K, d = self.ws, self.K, self.d
        self.emb = ws.alloc("bn.emb", K * d, torch.float32)[:K * d].view(K, d)
        self.ema_numer = ws.alloc("bn.ema_numer", K * d, torch.float32)[:K * d].view(K, d)
        self.ema_denom = ws.alloc("bn.ema_denom", K, torch.float32)[:K]
        # one buffer so that the data-parallel exchange of the EMA statistics is ONE all-reduce
        self.zn_sum = ws.alloc("bn.zn_sum", K * d + K, torch.float32)[:K * d + K]
        self.z_sum = self.zn_sum[:K * d].view(K, d)
        self.n_sum = self.zn_sum[K * d:]
        self.ind_hist = ws.alloc("bn.ind_hist", K, torch.float32)[:K]
        self.demb_ptr = None                                             # (the codebook takes no gradient)

    def _ema_op(self, z_sum: int, n_sum: int, update_codebook: int, gamma: float) -> "L.VqEma":
        em = L.VqEma()
        em.numer, em.denom = self.ema_numer.data_ptr(), self.ema_denom.data_ptr()
        em.z_sum, em.n_sum, em.emb = z_sum, n_sum, self.emb.data_ptr()
        em.K, em.d, em.update_codebook = self.K, self.d, update_codebook
        em.gamma, em.gamma_comp = gamma, float(1.0 - gamma)
        em.guard = self.guard_ptr
        return em

    def _forward(self, fa, fb):
        super()._forward(fa, fb)
        st = L.VqStats()
        st.ze, st.ind = self.lin.ptr, self.ind.data_ptr()
        st.Q, st.K, st.d, st.d_pitch = self.Q, self.K, self.d, self.nlin_p
        st.z_sum, st.n_sum, st.hist = self.z_sum.data_ptr(), self.n_sum.data_ptr(), self.ind_hist.data_ptr()
        fa.add(L.OP_VQ_STATS, st, "vq.stats", TAG_VQ)
        # the diagnostics op (side lane of fwd_b) reads this step's LOCAL code counts; a data-parallel
        # caller all-reduces zn_sum in place while fwd_b runs, so it gets its own copy
        self.n_sum_diag = self.ws.alloc("bn.n_sum_diag", self.K, torch.float32)
        ntbl = CopyTableBuilder(self.ws, "tbl.nsum")
        ntbl.add(self.n_sum.data_ptr(), self.n_sum_diag.data_ptr(), [self.K], [1], [1], F3, F3)
        ntbl.emit(fa, "n_sum -> diagnostics copy")
        # EMA runs at the START of part B (after the optional cross-rank sum); the
        # codebook refresh is deferred to after backward so that forward and backward
        # of one step see the same emb
        em = self._ema_op(self.z_sum.data_ptr(), self.n_sum.data_ptr(), 0, float(self.hps.bn_vq_ema_gamma))
        with fb.side(3):                                   # nothing in the forward / backward reads the accumulators
            fb.add(L.OP_VQ_EMA, em, "vq.ema", TAG_VQ)

    def _diag_op(self, w, scratch, out):
        dv = super()._diag_op(w, scratch, out)
        dv.hist, dv.n_sum = self.ind_hist.data_ptr(), self.n_sum_diag.data_ptr()
        return dv

    def loss_terms(self, nll):
        com = (self.min_dist.data_ptr(), self.Q, float(self.hps.bn_vq_gamma))
        return [com] if self.loss_mode == "head" else [nll, com]

    def nll_scale(self, scale):
        return 0.0 if self.loss_mode == "head" else scale

    def _usage_metrics(self, diag):
        return {"hst_ent": diag[4], "nunq": diag[5]}        # vqema_bn.py:258-260

    def build_codebook(self):
        """Deferred codebook refresh (vqema_bn.py:216-222): emb = numer / denom, the accumulators unchanged."""
        self.cb = Plan("codebook")
        z0 = self.ws.alloc("bn.zero_k", self.K * self.d, torch.float32)
        self.cb.add(L.OP_VQ_EMA, self._ema_op(z0.data_ptr(), z0.data_ptr(), 1, 1.0), "vq.codebook", TAG_VQ)

    def restart_op(self) -> Tuple[torch.Tensor, torch.Tensor, "L.VqRestart"]:
        """(int32 [4] counts, int32 [AEW_VQ_RESTART_MAX][2] pairs, the op over bn.lin / emb / ema_numer / ema_denom)."""
        out = self.ws.alloc("restart.out", 4, torch.int32)[:4]
        pairs = self.ws.alloc("restart.pairs", 2 * L.VQ_RESTART_MAX, torch.int32)[:2 * L.VQ_RESTART_MAX].view(L.VQ_RESTART_MAX, 2)
        rs = L.VqRestart()
        rs.ze, rs.Q, rs.d, rs.d_pitch = self.lin.ptr, self.Q, self.d, self.nlin_p
        rs.emb, rs.numer, rs.denom = self.emb.data_ptr(), self.ema_numer.data_ptr(), self.ema_denom.data_ptr()
        rs.K, rs.max_codes, rs.min_usage, rs.denom_init = self.K, 1, 0.0, 1.0
        rs.out, rs.pairs = out.data_ptr(), pairs.data_ptr()
        rs.guard = self.guard_ptr
        return out, pairs, rs


class VaeBottleneck(BottleneckPlan):
    """vae_bn.py:26-62, 76-125: sample = mu + eps * sigma; the loss is the mean NLL + anneal * max(KL, free nats)."""
    lin_outs = 2              # mu | logvar
    names = BottleneckPlan.names + ("eps", "kl_terms", "anneal_weight", "dp_world")

    def _alloc(self):
        ws, B, Ne, d = self.ws, self.B, self.g.embed_len, self.d
        self.code = Mat.new(ws, "bn.sample", B, Ne, self.dp, F3)
        self.eps = ws.alloc("bn.eps", self.Q * d, torch.float32)[:self.Q * d].view(B, Ne, d)
        self.kl_terms = ws.alloc("bn.kl_terms", self.Q, torch.float32)
        self.anneal_weight = 0.0
        self.dp_world = 1                                                # set by dp.DataParallel (see set_anneal_weight)
        self.anneal_buf = ws.alloc("bn.anneal", 4, torch.float32)[:1]   # read by the loss op
        self.anneal_bwd = ws.alloc("bn.anneal_bwd", 4, torch.float32)[:1]   # read by the KL-gradient op

    def _op(self, backward: bool, dcode: Optional[Mat] = None) -> "L.Vae":
        va = L.Vae()
        va.lin, va.lin_pitch, va.eps = self.lin.ptr, self.nlin_p, self.eps.data_ptr()
        va.Q, va.d, va.d_pitch = self.Q, self.d, self.dp
        va.sample, va.kl_terms = self.code.ptr, self.kl_terms.data_ptr()
        va.backward = int(backward)
        if backward:
            va.dsample = dcode.ptr
            va.kl_coef = float(self.anneal_weight)
            va.kl_coef_dev = self.anneal_bwd.data_ptr()
            va.kl_value = self.loss_ptr + 4 * 2                  # out[1 + term 1]
            va.free_nats = float(self.hps.bn_free_nats)
            va.dlin = self.dlin.ptr
            va.gmul = self.gmul_ptr
        return va

    def _forward(self, fa, fb):
        fa.add(L.OP_VAE, self._op(False), "vae.sample", TAG_VQ)

    def loss_terms(self, nll):
        return [nll, (self.kl_terms.data_ptr(), self.Q, -0.5)]

    def loss_op(self, nll):
        red = super().loss_op(nll)                               # the KL term clamped at the free nats, times the device-side
        red.clamp[1], red.clamp_min[1], red.post_scale[1] = 1, float(self.hps.bn_free_nats), 0.0     # anneal weight
        red.post_scale_dev[1] = self.anneal_buf.data_ptr()
        return red

    def metrics(self, met, diag, loss):
        return {"kl_div_loss": loss[2], "log_pred_loss": met[1]}

    def _backward(self, bw, dcode):
        bw.add(L.OP_VAE, self._op(True, dcode), "vae.bwd", TAG_VQ)


class AeBottleneck(BottleneckPlan):
    """ae_bn.py:11-16, 29-46: the code is the (biased) linear's output; the loss is the mean NLL + 0.001 * mean ||ze||^2."""
    lin_flags = L.EF_BIAS

    def _alloc(self):
        self.code = self.lin
        self.norm_terms = self.ws.alloc("bn.norm_terms", self.Q, torch.float32)
        bt = self.ws.alloc("bn.wp.bias", self.nlin_p, torch.float32)
        self.pk.pack_tbl.add(self.ps.ptr("bottleneck.linear.bias"), bt.data_ptr(), [self.d], [1], [1], F3, F3)
        self.lin_bias_ptr = bt.data_ptr()

    def _op(self, backward: bool, dcode: Optional[Mat] = None) -> "L.AeNorm":
        an = L.AeNorm()
        an.ze, an.Q, an.d, an.d_pitch = self.lin.ptr, self.Q, self.d, self.nlin_p
        an.term = self.norm_terms.data_ptr()
        an.backward = int(backward)
        if backward:
            an.dze_in, an.coef, an.dze = dcode.ptr, 0.001 / self.Q, self.dlin.ptr
            an.gmul = self.gmul_ptr
        return an

    def _forward(self, fa, fb):
        fa.add(L.OP_AE_NORM, self._op(False), "ae.norm", TAG_VQ)

    def loss_terms(self, nll):
        return [nll, (self.norm_terms.data_ptr(), self.Q, 0.001 / self.Q)]

    def metrics(self, met, diag, loss):
        return {"norm": loss[2]}

    def _backward(self, bw, dcode):
        bw.add(L.OP_AE_NORM, self._op(True, dcode), "ae.norm.bwd", TAG_VQ)
        cs = colsum_op(self.ws, self.dlin.seg(64), F3, self.g.embed_len, self.d, self.B,
                       self.ps.ptr("bottleneck.linear.bias", True), 0, "det.db.bn")
        with bw.side():
            bw.add(L.OP_COLSUM, cs, "db.bn", TAG_VQ)
