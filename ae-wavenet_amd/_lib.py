"""ctypes binding of the C ABI in include/aewavenet.h.

The structures below mirror the header field-for-field; `load()` checks their sizes against
`aew_sizeof()` so a drifted mirror fails loudly.  There is no CPU fallback: if the shared
library is missing, `load()` raises and nothing in the product path can run.
"""
from __future__ import annotations

import ctypes as C
import os

MAX_SEGS = 32
BF16, F32 = 0, 1

E_ARG, E_UNSUP, E_ALIGN = -1, -2, -3

EPI_STORE, EPI_GATED, EPI_RES_SKIP, EPI_DFG = 0, 1, 2, 3
EF_BIAS, EF_RELU, EF_OUT1_PRE, EF_ADD_AUX0 = 1 << 0, 1 << 1, 1 << 2, 1 << 3
EF_MUL_POS1, EF_OUT1_POS1, EF_ACCUM, EF_OUT2_RELU, EF_COUNT_ZERO = 1 << 4, 1 << 5, 1 << 6, 1 << 7, 1 << 8
EF_RELU_POST = 1 << 9
EF_OUT2_COPY = 1 << 10
NT_EPI_LINES_DEFAULT = 1            # the library's aew_set_nt_epi_lines default (csrc/aew_gemm.hip: AEW_NT_EPI_LINES_DEFAULT)

(OP_GEMM_NT, OP_GEMM_TN, OP_COPY_TABLE, OP_VQ_NEAREST, OP_VQ_STATS, OP_VQ_EMA, OP_VQ_BWD,
 OP_LC_GATHER, OP_LC_SCATTER, OP_SPK_BIAS, OP_SPK_BWD, OP_BASE_GATHER, OP_SOFTMAX_NLL, OP_COLSUM,
 OP_REDUCE, OP_ADAM, OP_ZERO, OP_VAE, OP_AE_NORM, OP_JITTER, OP_VQ_DIAG, OP_MFCC, OP_MOMENTS, OP_GEMM_TN_GROUP,
 OP_NT_CHAIN, OP_GRAD_NORM, OP_UPDATE_RATIO, OP_SWAP, OP_VQ_RESTART, OP_EVAL_ACC, OP_WINDOW_GATHER,
 OP_GRAD_WELFORD, OP_SEG_SELECT, OP_ACCUM, OP_CODE_LOOKUP, OP_CODE_RUNS, OP_ADAM_GROUPS, OP_EVAL_GROUPS,
 OP_MEL_TILE, OP_CODE_STITCH, OP_CODE_TILE, OP_COND_STITCH, OP_WAV_TILE, OP_NLL_STITCH, OP_SCORE_REDUCE, OP_SEQ_ALIGN,
 OP_FRAME_STITCH, OP_CODE_SEGMENT, OP_SEQ_SEARCH, OP_ABX_COUNT, OP_SEQ_DISCOVER) = range(1, 52)

vp, i32, i64, u32, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float


class Seg(C.Structure):
    _fields_ = [("ptr", vp), ("batch_stride", i64), ("row_pitch", i32), ("row_step", i32),
                ("row_off", i32), ("row_lo", i32), ("row_hi", i32), ("k_len", i32)]


class View(C.Structure):
    _fields_ = [("ptr", vp), ("batch_stride", i64), ("row_pitch", i32), ("row_step", i32),
                ("row_off", i32), ("row_lo", i32), ("row_hi", i32), ("dtype", i32)]


class GemmNT(C.Structure):
    _fields_ = [("dtype", i32), ("impl", i32), ("M", i32), ("N", i32), ("N_pad", i32),
                ("batch", i32), ("n_segs", i32), ("K_total", i32), ("seg", Seg * MAX_SEGS),
                ("W", vp), ("epi", i32), ("flags", u32), ("out0", View), ("out1", View),
                ("out2", View), ("aux0", View), ("aux1", View), ("bias", vp), ("bias_bs", i64),
                ("n_split", i32), ("reserved", i32), ("counter", vp),
                ("W2", vp), ("N2", i32), ("N2_pad", i32), ("out3", View),
                ("k_split", i32), ("pad2_", i32), ("ksplit_ws", vp), ("ksplit_tickets", vp)]


class NtPick(C.Structure):
    """aew_nt_pick_t: what the NT launcher decides for a descriptor (aew_nt_pick; test and measurement aid)."""
    _fields_ = [("kernel", i32), ("variant", i32), ("bm", i32), ("bn", i32), ("threads", i32), ("lds_bytes", i32),
                ("grid", i32), ("k_split", i32), ("dwp", i32), ("name", C.c_char * 96)]


class GemmTN(C.Structure):
    _fields_ = [("dtype", i32), ("impl", i32), ("Mc", i32), ("batch", i32), ("N", i32),
                ("N_pad", i32), ("g", Seg), ("n_segs", i32), ("K_total", i32),
                ("seg", Seg * MAX_SEGS), ("out", vp), ("out_batch_stride", i64),
                ("snap_out", vp), ("snap_bs", i64), ("snap_k", i32), ("pad_", i32), ("colsum_out", vp),
                ("grp_splits", i32), ("grp_rows", i32)]


class TnPick(C.Structure):
    """aew_tn_pick_t: what the TN launchers decide for an op or a grouped launch (aew_tn_pick / aew_tn_group_pick)."""
    _fields_ = [(n, i32) for n in "row bk bn threads lds_bytes".split()] + [("grid", i32 * 3)] + [(n, i32) for n in "tile rc splits rows_per_split fold slabs cursor cursor_epoch cursor_slack".split()] + [("name", C.c_char * 96)]


class GemmTNGroup(C.Structure):
    _fields_ = [("descs", vp), ("tile_map", vp), ("n_descs", i32), ("n_blocks", i32), ("tile", i32), ("cursor_stride", i32),
                ("cursors", vp)]


CHAIN_MAXDEP = 3


class ChainDep(C.Structure):
    _fields_ = [("cnt_base", i32), ("n_mt", i32), ("need", i32), ("d_lo", i32), ("d_hi", i32), ("c_lo", i32), ("c_hi", i32),
                ("bm", i32)]


class NtStage(C.Structure):
    """aew_nt_stage_t: one stage of a chained NT launch (filled in by aew_nt_chain_build, uploaded to device memory)."""
    _fields_ = [("g", GemmNT), ("kind", i32), ("first_block", i32), ("n_blocks", i32), ("n_mt", i32), ("n_nt", i32),
                ("cnt_base", i32), ("publish", i32), ("n_deps", i32), ("dep", ChainDep * CHAIN_MAXDEP)]


class NtChain(C.Structure):
    _fields_ = [("stages", vp), ("block_stage", vp), ("counters", vp), ("n_stages", i32), ("n_blocks", i32),
                ("n_counters", i32), ("set", i32), ("n_ops", i32), ("spin_max", i32), ("flags", i32), ("built_window", i32),
                ("sticky", vp)]


class CopyRec(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("dims", i32 * 4), ("ss", i64 * 4), ("ds", i64 * 4),
                ("src_dtype", i32), ("dst_dtype", i32), ("red_n", i32), ("accumulate", i32),
                ("red_stride", i64), ("scale", f32), ("first_block", i32), ("tr_a", i32), ("tr_b", i32)]


class CopyTable(C.Structure):
    _fields_ = [("recs", vp), ("block_rec", vp), ("n_blocks", i32), ("n_recs", i32)]


class VqNearest(C.Structure):
    _fields_ = [("ze", vp), ("emb", vp), ("Q", i32), ("K", i32), ("d", i32), ("d_pitch", i32),
                ("metric", i32), ("ind", vp), ("dist", vp), ("zq", vp), ("scratch", vp), ("n_split", i32)]


class VqStats(C.Structure):
    _fields_ = [("ze", vp), ("ind", vp), ("Q", i32), ("K", i32), ("d", i32), ("d_pitch", i32),
                ("z_sum", vp), ("n_sum", vp), ("hist", vp)]


class VqEma(C.Structure):
    _fields_ = [("numer", vp), ("denom", vp), ("z_sum", vp), ("n_sum", vp), ("emb", vp),
                ("K", i32), ("d", i32), ("update_codebook", i32), ("gamma", f32),
                ("gamma_comp", f32), ("guard", vp)]


class VqBwd(C.Structure):
    _fields_ = [("ze", vp), ("emb", vp), ("ind", vp), ("dzq", vp), ("Q", i32), ("d", i32),
                ("d_pitch", i32), ("metric", i32), ("coef", f32), ("demb_coef", f32),
                ("dze", vp), ("demb", vp), ("gmul", vp)]


class LcGather(C.Structure):
    _fields_ = [("src", vp), ("src_bs", i64), ("src_pitch", i32), ("jitter", vp),
                ("jit_pitch", i32), ("dst", vp), ("dst_bs", i64), ("dst_pitch", i32),
                ("B", i32), ("N", i32), ("C", i32), ("C_pad", i32), ("take_compat", i32)]


class LcScatter(C.Structure):
    _fields_ = [("d", vp), ("d_bs", i64), ("d_pitch", i32), ("jitter", vp), ("jit_pitch", i32),
                ("dsrc", vp), ("dsrc_bs", i64), ("dsrc_pitch", i32), ("B", i32), ("N", i32),
                ("C", i32), ("take_compat", i32)]


class SpkBias(C.Structure):
    _fields_ = [("params", vp), ("voice", vp), ("off_bias_sig", vp), ("off_bias_gate", vp),
                ("off_proj_sig", vp), ("off_proj_gate", vp), ("off_spk_w", i64),
                ("off_spk_b", i64), ("B", i32), ("L", i32), ("D", i32), ("D_pad", i32),
                ("C_lc", i32), ("G", i32), ("n_speakers", i32), ("bias", vp), ("gc", vp)]


class SpkBwd(C.Structure):
    _fields_ = [("params", vp), ("voice", vp), ("off_bias_sig", vp), ("off_bias_gate", vp),
                ("off_proj_sig", vp), ("off_proj_gate", vp), ("off_spk_w", i64),
                ("off_spk_b", i64), ("B", i32), ("L", i32), ("D", i32), ("D_pad", i32),
                ("C_lc", i32), ("G", i32), ("n_speakers", i32), ("colsum", vp), ("gc", vp),
                ("grads", vp), ("colsum_running", i32), ("layer_range", i32), ("det_scratch", vp), ("det_tickets", vp)]


class Tuning(C.Structure):
    """aew_tuning_t: kernel-shape choices as a record (the aew_set_* switches edit the process-wide one; Plan.run(...,
    tuning=...) / aew_run_plan_tuned apply a caller's own to one call)."""
    _fields_ = [("nt_wave_rows", i32), ("nt_pipe", i32), ("nt_rows192", i32), ("nt_small_tiles", i32), ("nt_small_n64", i32), ("nt_small_w8", i32), ("nt_small_deep", i32), ("nt_window", i32), ("nt_mem128", i32), ("nt_deep", i32), ("nf_loaders", i32), ("nf_deep", i32), ("fn_enable", i32), ("fn_ring3", i32), ("tn_safe", i32), ("tn_big", i32), ("tn_big_target", i32), ("tn_fold_rows", i32), ("tn_target_blocks", i32), ("tn_small_tiles", i32), ("tn_small_target", i32), ("lanes", i32), ("tn_cursor_epoch", i32), ("tn_cursor_slack", i32), ("nt_chain", i32), ("deterministic", i32), ("tn_mfma32", i32), ("reserved_", i32 * 5)]


class BaseGather(C.Structure):
    _fields_ = [("wav", vp), ("wav_pitch", i32), ("wav_off", i32), ("W", vp), ("bias", vp),
                ("Wt", vp), ("B", i32), ("T", i32), ("R", i32), ("R_pad", i32), ("Q", i32), ("x", vp),
                ("x_bs", i64), ("x_pitch", i32), ("onehot", vp), ("oh_bs", i64),
                ("oh_pitch", i32), ("Q_pad", i32), ("ones_channel", i32)]


class SoftmaxNll(C.Structure):
    _fields_ = [("logits", vp), ("bs", i64), ("pitch", i32), ("wav", vp), ("wav_pitch", i32),
                ("tgt_off", i32), ("B", i32), ("w", i32), ("Q", i32), ("Q_pad", i32),
                ("nll", vp), ("ptgt", vp), ("dlogits", vp), ("dl_bs", i64), ("dl_pitch", i32),
                ("scale", f32), ("backward", i32), ("gmul", vp), ("peak", vp), ("amax", vp)]


class Colsum(C.Structure):
    _fields_ = [("x", Seg), ("dtype", i32), ("M", i32), ("N", i32), ("batch", i32),
                ("out", vp), ("out_bs", i64), ("accumulate", i32), ("pad_", i32), ("det_scratch", vp), ("det_tickets", vp)]


class Reduce(C.Structure):
    _fields_ = [("x", vp * 4), ("n", i32 * 4), ("scale", f32 * 4), ("clamp", i32 * 4),
                ("clamp_min", f32 * 4), ("post_scale", f32 * 4), ("n_terms", i32), ("out", vp),
                ("post_scale_dev", vp * 4)]


class Adam(C.Structure):
    _fields_ = [("p", vp), ("g", vp), ("m", vp), ("v", vp), ("n", i64), ("lr", f32),
                ("beta1", f32), ("beta2", f32), ("eps", f32), ("bc1", f32), ("bc2", f32),
                ("grad_scale", f32), ("pad_", i32), ("guard", vp), ("clip", vp), ("track", vp),
                ("avg", vp), ("avg_rate", f32), ("pad2_", i32)]


class AdamTensor(C.Structure):
    """aew_adam_tensor_t: one tensor's record of a grouped Adam launch (decay = fp32(1 - lr * weight_decay), in double)."""
    _fields_ = [("lr", f32), ("decay", f32), ("frozen", i32), ("pad_", i32)]


class AdamGroups(C.Structure):
    """aew_adam_groups_t: the HOST record AdamGrouped.groups points at (keep it alive while a plan holds its address)."""
    _fields_ = [("chunks", vp), ("chunks_host", vp), ("n_chunks", i64), ("tensors", vp), ("n_tensors", i32), ("pad_", i32),
                ("base", i64)]


class AdamGrouped(C.Structure):
    """aew_adam_grouped_t (AEW_OP_ADAM_GROUPS): the Adam descriptor and the record of its parameter groups."""
    _fields_ = [("adam", Adam), ("groups", vp)]


class Swap(C.Structure):
    """aew_swap_t: exchange two flat fp32 buffers in place (the parameters and their average, Adam.avg)."""
    _fields_ = [("a", vp), ("b", vp), ("n", i64)]


ACCUM_FIRST, ACCUM_ADD, ACCUM_LAST = 0, 1, 2


class Accum(C.Structure):
    """aew_accum_t: fold the buffer a backward just wrote into a running sum (FIRST: acc = g, ADD: acc += g, LAST: g += acc)."""
    _fields_ = [("acc", vp), ("g", vp), ("n", i64), ("mode", i32), ("pad_", i32)]


class CodeLookup(C.Structure):
    """aew_code_lookup_t: zq[q] = emb[ind[q]] (pad channels zero); an index outside [0, K) gives a zero row and counts in *bad."""
    _fields_ = [("ind", vp), ("emb", vp), ("zq", vp), ("bad", vp), ("Q", i32), ("K", i32), ("d", i32), ("d_pitch", i32)]


class CodeRuns(C.Structure):
    """aew_code_runs_t: run-length collapse of code rows: units (-1 behind the last run), lengths (0 behind it), n_runs."""
    _fields_ = [("ind", vp), ("ind_pitch", i64), ("units", vp), ("lengths", vp), ("n_runs", vp), ("B", i32), ("N", i32)]


class UttRow(C.Structure):
    """aew_utt_row_t: one batch row of a whole-utterance encode - where its window starts in the ragged mel buffer, how many
    frames exist there, where its codes go and how many of them are stored.  UTT_ROW_DTYPE is the same record for numpy."""
    _fields_ = [("src", i64), ("dst", i64), ("pitch", i32), ("avail", i32), ("n_valid", i32), ("pad_", i32)]


UTT_ROW_DTYPE = [("src", "<i8"), ("dst", "<i8"), ("pitch", "<i4"), ("avail", "<i4"), ("n_valid", "<i4"), ("pad_", "<i4")]


class MelTile(C.Structure):
    """aew_mel_tile_t: in_mel[b] = the window of table[first_row + b] cut out of the ragged mel buffer, zeros behind it."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("mel", vp), ("n_src", i64),
                ("in_mel", vp), ("n_mel", i32), ("mel_len", i32)]


class CodeStitch(C.Structure):
    """aew_code_stitch_t: the first n_valid codes (and distances) of each batch row to their place in the ragged outputs."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("ind", vp), ("min_dist", vp),
                ("codes", vp), ("dist", vp), ("n_dst", i64), ("E", i32), ("pad_", i32)]


class CondRow(C.Structure):
    """aew_cond_row_t: one batch row of a whole-utterance conditioning - where its window starts in the flat code buffer
    and which of its codes exist, which rows of its cond it owns and where they go, its voice, whether it is the first
    window of its utterance.  COND_ROW_DTYPE is the same record for numpy."""
    _fields_ = [("code0", i64), ("utt", i32), ("stream", i32), ("lo", i32), ("hi", i32), ("src_row", i32), ("n_rows", i32),
                ("dst_row", i32), ("pitch", i32), ("voice", i32), ("first", i32)]


COND_ROW_DTYPE = [("code0", "<i8"), ("utt", "<i4"), ("stream", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("src_row", "<i4"),
                  ("n_rows", "<i4"), ("dst_row", "<i4"), ("pitch", "<i4"), ("voice", "<i4"), ("first", "<i4")]


class CodeTile(C.Structure):
    """aew_code_tile_t: ind[b] / in_voice[b] = the window of table[first_row + b] cut out of the flat code buffer, code 0
    where the utterance has none; codes outside [0, K) become 0 and are counted in *bad."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("codes", vp), ("n_codes", i64),
                ("ind", vp), ("in_voice", vp), ("bad", vp), ("E", i32), ("K", i32), ("n_voice", i32), ("pad_", i32)]


class CondStitch(C.Structure):
    """aew_cond_stitch_t: the cond rows each batch row owns (and its gated bias, for a first window) to their stream."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("cond", vp), ("cond_bs", i64),
                ("cond_pitch", i32), ("T", i32), ("cond_utt", vp), ("n_dst", i64), ("bias", vp), ("bias_utt", vp),
                ("Cp", i32), ("bias_n", i32), ("n_streams", i32), ("pad_", i32)]


class ScoreRow(C.Structure):
    """aew_score_row_t: one batch row of a whole-utterance scoring - where its window starts in the flat code buffer and
    which of its codes exist, the utterance's samples in the flat waveform buffer and the one that is the window's
    decoder-input row 0, its voice, which outputs it owns and where they go.  SCORE_ROW_DTYPE is the same record for
    numpy."""
    _fields_ = [("code0", i64), ("wav_base", i64), ("wav_len", i64), ("wav0", i64), ("dst", i64), ("utt", i32), ("lo", i32),
                ("hi", i32), ("voice", i32), ("src", i32), ("n_out", i32)]


SCORE_ROW_DTYPE = [("code0", "<i8"), ("wav_base", "<i8"), ("wav_len", "<i8"), ("wav0", "<i8"), ("dst", "<i8"), ("utt", "<i4"),
                   ("lo", "<i4"), ("hi", "<i4"), ("voice", "<i4"), ("src", "<i4"), ("n_out", "<i4")]


class WavTile(C.Structure):
    """aew_wav_tile_t: wav[b][wav_off : wav_off + T] / ind[b] / in_voice[b] = the window of table[first_row + b] cut out of
    the flat waveform and code buffers; the zero-amplitude code / code 0 where the utterance has nothing, and for values
    outside [0, n_quant) / [0, K), which are counted in *bad_wav / *bad_codes."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("codes", vp), ("n_codes", i64),
                ("wavs", vp), ("n_wav", i64), ("ind", vp), ("in_voice", vp), ("wav", vp), ("bad_codes", vp), ("bad_wav", vp),
                ("wav_pitch", i32), ("wav_off", i32), ("T", i32), ("n_quant", i32), ("E", i32), ("K", i32), ("n_voice", i32),
                ("zero", f32)]


class NllStitch(C.Structure):
    """aew_nll_stitch_t: the per-position nll (and ptgt, and the top-1 hit) of the outputs each batch row owns to the flat
    per-utterance arrays."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("nll", vp), ("ptgt", vp), ("amax", vp),
                ("logits", vp), ("bs", i64), ("wav", vp), ("dst_nll", vp), ("dst_ptgt", vp), ("dst_hit", vp), ("n_dst", i64),
                ("pitch", i32), ("n_quant", i32), ("wav_pitch", i32), ("tgt_off", i32), ("w", i32), ("pad_", i32)]


class ScoreReduce(C.Structure):
    """aew_score_reduce_t: per utterance (n, sum nll, sum ptgt, sum hit) as doubles in aew_eval_acc_t's order, and the
    four means as fp32."""
    _fields_ = [("offsets", vp), ("offsets_host", vp), ("nll", vp), ("ptgt", vp), ("hit", vp), ("n_src", i64), ("acc", vp),
                ("out", vp), ("U", i32), ("pad_", i32)]


# the columns of aew_score_reduce_t's `out` and the accessors of codes.UtteranceScores derived from them (the first is not
# "nll": that is the flat per-sample tensor)
SCORE_OUT_NAMES = ("nll_per_sample", "bits_per_sample", "top1", "mean_prob")


ALIGN_DTW, ALIGN_EDIT = 0, 1
ALIGN_EUCLID, ALIGN_SQEUCLID = 0, 1
ALIGN_MAX_D, ALIGN_MAX_LEN = 256, 1 << 20


class AlignSeq(C.Structure):
    """aew_align_seq_t: one sequence inside a side's buffer - element (i, k) is feat[base + i * frame_stride + k * chan_stride].
    ALIGN_SEQ_DTYPE is the same record for numpy."""
    _fields_ = [("base", i64), ("frame_stride", i64), ("chan_stride", i64), ("len", i32), ("pad_", i32)]


ALIGN_SEQ_DTYPE = [("base", "<i8"), ("frame_stride", "<i8"), ("chan_stride", "<i8"), ("len", "<i4"), ("pad_", "<i4")]


class AlignPair(C.Structure):
    """aew_align_pair_t: which A-side and B-side sequences a pair compares, where its n * m back-pointer bytes and its
    n + m - 1 path entries start.  ALIGN_PAIR_DTYPE is the same record for numpy."""
    _fields_ = [("a", i32), ("b", i32), ("back_base", i64), ("path_base", i64)]


ALIGN_PAIR_DTYPE = [("a", "<i4"), ("b", "<i4"), ("back_base", "<i8"), ("path_base", "<i8")]


class SeqAlign(C.Structure):
    """aew_seq_align_t: DTW (cost, steps, optional back-pointers and path) or the edit distance of n_pairs pairs of
    sequences, one wavefront per pair; the tables as device and host copies."""
    _fields_ = [("mode", i32), ("metric", i32), ("D", i32), ("n_pairs", i32), ("seq_a", vp), ("seq_a_host", vp),
                ("seq_b", vp), ("seq_b_host", vp), ("pairs", vp), ("pairs_host", vp), ("n_a", i32), ("n_b", i32),
                ("feat_a", vp), ("feat_b", vp), ("n_feat_a", i64), ("n_feat_b", i64), ("cost", vp), ("steps", vp), ("bad", vp),
                ("ws", vp), ("ws_bytes", i64), ("back", vp), ("n_back", i64), ("path", vp), ("n_path", i64)]


SEARCH_MEAN, SEARCH_COST = 0, 1
SEARCH_MAX_HITS = 32


class SearchPair(C.Structure):
    """aew_search_pair_t: which query and which document a pair searches, where the document's m profile entries start.
    SEARCH_PAIR_DTYPE is the same record for numpy."""
    _fields_ = [("a", i32), ("b", i32), ("prof_base", i64)]


SEARCH_PAIR_DTYPE = [("a", "<i4"), ("b", "<i4"), ("prof_base", "<i8")]


class SeqSearch(C.Structure):
    """aew_seq_search_t: subsequence DTW of n_pairs (query, document) pairs - the per-end profile (cost, steps, start) and
    the n_hits best non-overlapping matches of each; the tables as device and host copies."""
    _fields_ = [("metric", i32), ("rank", i32), ("D", i32), ("n_pairs", i32), ("n_hits", i32), ("min_len", i32),
                ("max_len", i32), ("pad_", i32), ("seq_a", vp), ("seq_a_host", vp), ("seq_b", vp), ("seq_b_host", vp),
                ("pairs", vp), ("pairs_host", vp), ("n_a", i32), ("n_b", i32), ("feat_a", vp), ("feat_b", vp),
                ("n_feat_a", i64), ("n_feat_b", i64), ("prof_cost", vp), ("prof_steps", vp), ("prof_start", vp),
                ("n_prof", i64), ("hits", vp), ("hit_cost", vp), ("hit_steps", vp), ("count", vp), ("bad", vp),
                ("ws", vp), ("ws_bytes", i64)]


class DiscoverPair(C.Structure):
    """aew_discover_pair_t: which two sequences a pair aligns locally, its band (cells with j - i < band are dead) and
    where its n profile entries start.  DISCOVER_PAIR_DTYPE is the same record for numpy."""
    _fields_ = [("a", i32), ("b", i32), ("band", i32), ("pad_", i32), ("prof_base", i64)]


DISCOVER_PAIR_DTYPE = [("a", "<i4"), ("b", "<i4"), ("band", "<i4"), ("pad_", "<i4"), ("prof_base", "<i8")]


class SeqDiscover(C.Structure):
    """aew_seq_discover_t: local-alignment DTW of n_pairs pairs - the per-row profile (score, end column, origin row,
    origin column, steps) and the n_hits best alignments of each whose A ranges do not overlap; the tables as device and
    host copies."""
    _fields_ = [("metric", i32), ("n_hits", i32), ("D", i32), ("n_pairs", i32), ("min_len", i32), ("max_len", i32),
                ("threshold", f32), ("pad_", i32), ("seq_a", vp), ("seq_a_host", vp), ("seq_b", vp), ("seq_b_host", vp),
                ("pairs", vp), ("pairs_host", vp), ("n_a", i32), ("n_b", i32), ("feat_a", vp), ("feat_b", vp),
                ("n_feat_a", i64), ("n_feat_b", i64), ("prof_score", vp), ("prof_end", vp), ("prof_row", vp),
                ("prof_col", vp), ("prof_steps", vp), ("n_prof", i64), ("hits", vp), ("hit_score", vp), ("hit_steps", vp),
                ("count", vp), ("bad", vp), ("ws", vp), ("ws_bytes", i64)]


ABX_WITHIN, ABX_ACROSS = 0, 1
ABX_MAX_N = 16384


class AbxGroup(C.Structure):
    """aew_abx_group_t: one non-empty (category, speaker) group - its sorted positions [lo, hi), its category and speaker
    indices.  ABX_GROUP_DTYPE is the same record for numpy."""
    _fields_ = [("lo", i32), ("hi", i32), ("cat", i32), ("spk", i32)]


ABX_GROUP_DTYPE = [("lo", "<i4"), ("hi", "<i4"), ("cat", "<i4"), ("spk", "<i4")]


class AbxCount(C.Structure):
    """aew_abx_count_t: per sorted position x and group g the number of (A, B, X) triples and twice the wrong ones over
    an N x N distance matrix read through the permutation; the three tables as device and host copies."""
    _fields_ = [("mode", i32), ("N", i32), ("G", i32), ("C", i32), ("S", i32), ("pad_", i32), ("ld", i64), ("dist", vp),
                ("perm", vp), ("perm_host", vp), ("groups", vp), ("groups_host", vp), ("partner", vp),
                ("partner_host", vp), ("n", vp), ("wrong2", vp)]


SEG_MAX_K, SEG_MAX_D = 4096, 4096


class SegUtt(C.Structure):
    """aew_seg_utt_t: one utterance of a segmentation - its rows in the ragged frame buffer (and in codes / dist), the
    first 64-bit word of its n_frames * (ceil(K / 64) + 1) in the workspace's back region, its switch penalty.
    SEG_UTT_DTYPE is the same record for numpy."""
    _fields_ = [("first_frame", i64), ("back_base", i64), ("n_frames", i32), ("lam", f32)]


SEG_UTT_DTYPE = [("first_frame", "<i8"), ("back_base", "<i8"), ("n_frames", "<i4"), ("lam", "<f4")]


class FrameStitch(C.Structure):
    """aew_frame_stitch_t: the first n_valid encoder-output rows of each batch row to their place in the ragged frame
    buffer (the aew_utt_row_t table of the code stitch)."""
    _fields_ = [("table", vp), ("table_host", vp), ("first_row", i32), ("B", i32), ("lin", vp), ("lin_bs", i64),
                ("frames", vp), ("n_dst", i64), ("E", i32), ("d_pitch", i32)]


class CodeSegment(C.Structure):
    """aew_code_segment_t: penalised Viterbi decoding of U utterances' frames over the K codebook entries - codes, their
    distances, the total cost and the segment count of each; the table as device and host copies."""
    _fields_ = [("frames", vp), ("n_elems", i64), ("emb", vp), ("K", i32), ("d", i32), ("d_pitch", i32), ("metric", i32),
                ("table", vp), ("table_host", vp), ("U", i32), ("pad_", i32), ("codes", vp), ("dist", vp), ("n_out", i64),
                ("cost", vp), ("n_seg", vp), ("n_bad", vp), ("ws", vp), ("ws_bytes", i64)]


VQ_RESTART_MAX = 1024


class VqRestart(C.Structure):
    """aew_vq_restart_t: re-seed the codes whose EMA count fell under min_usage from rows of this step's encoder outputs."""
    _fields_ = [("ze", vp), ("Q", i32), ("d", i32), ("d_pitch", i32), ("emb", vp), ("numer", vp), ("denom", vp),
                ("K", i32), ("max_codes", i32), ("min_usage", f32), ("denom_init", f32),
                ("seed", C.c_uint64), ("call", C.c_uint64), ("out", vp), ("pairs", vp), ("guard", vp)]


EVAL_ACC_N, EVAL_OUT_N = 16, 16
# finalize's out[i] by name (aew_eval_acc_t; Evaluator.result() hands them out under these names)
EVAL_OUT_NAMES = ("loss", "nll", "bits_per_sample", "top1", "tprb", "dist", "code_entropy", "code_perplexity", "codes_used",
                  "term1", "term2", "term3", "term4", "positions", "batches")


class EvalAcc(C.Structure):
    """aew_eval_acc_t: fold one evaluated batch into the running record on the device / turn the record into means."""
    _fields_ = [("nll", vp), ("ptgt", vp), ("wav", vp), ("wav_pitch", i32), ("tgt_off", i32), ("B", i32), ("w", i32),
                ("amax", vp), ("logits", vp), ("bs", i64), ("pitch", i32), ("n_quant", i32), ("ind", vp), ("dist", vp),
                ("Q", i32), ("K", i32), ("loss", vp), ("acc", vp), ("hist", vp), ("finalize", i32), ("pad_", i32), ("out", vp)]


EVAL_GACC_N, EVAL_GOUT_N, EVAL_TOUT_N = 8, 12, 16
# finalize's gout[g][i] / tout[i] by name (aew_eval_groups_t; Evaluator.by_group() / information() hand them out under these)
EVAL_GOUT_NAMES = ("windows", "positions", "nll", "bits_per_sample", "top1", "tprb", "dist", "queries", "code_entropy",
                   "code_perplexity", "codes_used")
EVAL_TOUT_NAMES = ("n", "code_entropy", "group_entropy", "cond_entropy", "mutual_information", "mutual_information_mm",
                   "mi_over_group_entropy", "mi_over_code_entropy", "cells", "groups_used", "codes_used", "dropped_windows",
                   "batches")


class EvalGroups(C.Structure):
    """aew_eval_groups_t: fold one evaluated batch into the per-group record and the (group, code) table / finalize them."""
    _fields_ = [("nll", vp), ("ptgt", vp), ("wav", vp), ("wav_pitch", i32), ("tgt_off", i32), ("B", i32), ("w", i32),
                ("amax", vp), ("logits", vp), ("bs", i64), ("pitch", i32), ("n_quant", i32), ("ind", vp), ("dist", vp),
                ("Qw", i32), ("K", i32), ("group", vp), ("G", i32), ("finalize", i32), ("gacc", vp), ("ghist", vp),
                ("gtot", vp), ("win", vp), ("gout", vp), ("tout", vp), ("scratch", vp)]


class WindowGather(C.Structure):
    """aew_window_gather_t: cut the next batch's windows out of the device-resident corpus (corpus.DeviceCorpus)."""
    _fields_ = [("snd", vp), ("n_snd", i64), ("snd_bytes", i32), ("B", i32), ("starts", vp), ("voices", vp), ("N", i64),
                ("order", vp), ("n_order", i32), ("num_replicas", i32), ("rank", i32), ("advance", i32), ("counter", vp),
                ("slice_size", i32), ("wav_pitch", i32), ("wav", vp), ("voice", vp), ("index", vp), ("position", vp)]


class GradWelford(C.Structure):
    """aew_grad_welford_t: fold one gradient sample into the running mean / sum of squared deviations (flat fp32 buffers)."""
    _fields_ = [("g", vp), ("mu", vp), ("s", vp), ("n", i64), ("first", i32), ("divisor", f32), ("chunks", vp),
                ("chunks_host", vp), ("n_chunks", i64), ("part", vp)]


SELECT_MAX_Q = 8


class SegSelect(C.Structure):
    """aew_seg_select_t: exact k-th smallest per tensor of a flat buffer, up to SELECT_MAX_Q ranks per tensor at once."""
    _fields_ = [("s", vp), ("chunks", vp), ("n_chunks", i64), ("n_tensors", i32), ("Q", i32), ("k", vp), ("out", vp),
                ("denom", f32), ("raw", i32), ("scratch", vp)]


UW_CHUNK = 4096


class UwChunk(C.Structure):
    """aew_uw_chunk_t: one chunk of the flat parameter buffer (never crosses a tensor boundary, no pad elements)."""
    _fields_ = [("off", i64), ("len", i32), ("tensor", i32)]


class UwTrack(C.Structure):
    """aew_uw_track_t: the HOST record Adam.track points at (keep it alive while a plan holds its address)."""
    _fields_ = [("chunks", vp), ("chunks_host", vp), ("n_chunks", i64), ("part", vp), ("base", i64), ("zero", i32),
                ("pad_", i32)]


class UpdateRatio(C.Structure):
    """aew_update_ratio_t: the chunk sums of a tracked Adam step -> per-tensor update norm, weight norm and their ratio."""
    _fields_ = [("part", vp), ("first", vp), ("n_tensors", i32), ("finalize", i32), ("add_in", vp), ("sums", vp),
                ("out", vp)]


GRAD_NORM_CHUNK, GRAD_NORM_MAX_RANGES = 16384, 8


class GradNorm(C.Structure):
    """aew_grad_norm_t: deterministic sum of squares over ranges of the flat gradient buffer + the clip coefficient
    Adam.clip reads (out[1..2])."""
    _fields_ = [("x", vp * GRAD_NORM_MAX_RANGES), ("n", i64 * GRAD_NORM_MAX_RANGES), ("n_ranges", i32), ("finalize", i32),
                ("add_in", vp), ("sumsq", vp), ("max_norm", f32), ("grad_scale", f32), ("eps", f32), ("pad_", i32),
                ("out", vp), ("scratch", vp), ("ticket", vp), ("guard", vp)]


class Zero(C.Structure):
    _fields_ = [("ptr", vp), ("bytes", i64)]


class Vae(C.Structure):
    _fields_ = [("lin", vp), ("lin_pitch", i32), ("eps", vp), ("Q", i32), ("d", i32),
                ("d_pitch", i32), ("sample", vp), ("kl_terms", vp), ("dsample", vp),
                ("kl_coef", f32), ("kl_value", vp), ("free_nats", f32), ("dlin", vp),
                ("backward", i32), ("kl_coef_dev", vp), ("gmul", vp)]


class AeNorm(C.Structure):
    _fields_ = [("ze", vp), ("Q", i32), ("d", i32), ("d_pitch", i32), ("term", vp),
                ("dze_in", vp), ("coef", f32), ("dze", vp), ("backward", i32), ("gmul", vp)]


class Jitter(C.Structure):
    _fields_ = [("out", vp), ("out_pitch", i32), ("B", i32), ("n", i32), ("p", f32), ("mode", i32),
                ("seed", C.c_uint64), ("step", C.c_uint64)]


class VqDiag(C.Structure):
    _fields_ = [("ze", vp), ("Q", i32), ("d", i32), ("d_pitch", i32), ("emb", vp), ("K", i32), ("hist", vp),
                ("n_sum", vp), ("logits", vp), ("bs", i64), ("pitch", i32), ("B", i32), ("w", i32),
                ("n_quant", i32), ("scratch", vp), ("out", vp), ("peak", vp), ("amax", vp)]


class Mfcc(C.Structure):
    _fields_ = [("wav", vp), ("wav_bs", i64), ("n", i32), ("B", i32), ("win", i32), ("hop", i32), ("n_bins", i32),
                ("n_mels", i32), ("n_mfcc", i32), ("left_pad", i32), ("trim_left", i32), ("trim_right", i32),
                ("n_frames", i32), ("window", vp), ("twiddle", vp), ("melw", vp), ("dct", vp), ("sg", vp),
                ("scratch", vp), ("out", vp), ("out_bs", i64), ("out_pitch", i32)]


class Moments(C.Structure):
    _fields_ = [("x", View), ("rows", i32), ("cols", i32), ("batch", i32), ("out", vp)]


class _OpU(C.Union):
    _fields_ = [("nt", GemmNT), ("tn", GemmTN), ("copy", CopyTable), ("vqn", VqNearest),
                ("vqs", VqStats), ("vqe", VqEma), ("vqb", VqBwd), ("lcg", LcGather),
                ("lcs", LcScatter), ("spk", SpkBias), ("spkb", SpkBwd), ("base", BaseGather),
                ("sm", SoftmaxNll), ("cs", Colsum), ("red", Reduce), ("adam", Adam),
                ("zero", Zero), ("vae", Vae), ("aen", AeNorm), ("jit", Jitter), ("diag", VqDiag), ("mfcc", Mfcc),
                ("mom", Moments), ("tng", GemmTNGroup), ("chain", NtChain), ("gnorm", GradNorm),
                ("ratio", UpdateRatio), ("swap", Swap), ("vqr", VqRestart), ("eva", EvalAcc), ("wgat", WindowGather),
                ("gwel", GradWelford), ("ssel", SegSelect), ("accum", Accum), ("clk", CodeLookup), ("crun", CodeRuns),
                ("adamg", AdamGrouped), ("evg", EvalGroups), ("mtile", MelTile), ("cstitch", CodeStitch),
                ("ctile", CodeTile), ("cndst", CondStitch), ("wtile", WavTile), ("nllst", NllStitch), ("sred", ScoreReduce),
                ("align", SeqAlign), ("fstitch", FrameStitch), ("cseg", CodeSegment), ("search", SeqSearch),
                ("abx", AbxCount), ("discover", SeqDiscover)]


class Op(C.Structure):
    _fields_ = [("kind", i32), ("tag", i32), ("lane", i32), ("join", i32), ("u", _OpU)]


OP_FIELD = {OP_GEMM_NT: "nt", OP_GEMM_TN: "tn", OP_COPY_TABLE: "copy", OP_VQ_NEAREST: "vqn",
            OP_VQ_STATS: "vqs", OP_VQ_EMA: "vqe", OP_VQ_BWD: "vqb", OP_LC_GATHER: "lcg",
            OP_LC_SCATTER: "lcs", OP_SPK_BIAS: "spk", OP_SPK_BWD: "spkb",
            OP_BASE_GATHER: "base", OP_SOFTMAX_NLL: "sm", OP_COLSUM: "cs", OP_REDUCE: "red",
            OP_ADAM: "adam", OP_ZERO: "zero", OP_VAE: "vae", OP_AE_NORM: "aen", OP_JITTER: "jit",
            OP_VQ_DIAG: "diag", OP_MFCC: "mfcc", OP_MOMENTS: "mom", OP_GEMM_TN_GROUP: "tng", OP_NT_CHAIN: "chain",
            OP_GRAD_NORM: "gnorm", OP_UPDATE_RATIO: "ratio", OP_SWAP: "swap", OP_VQ_RESTART: "vqr", OP_EVAL_ACC: "eva",
            OP_WINDOW_GATHER: "wgat", OP_GRAD_WELFORD: "gwel", OP_SEG_SELECT: "ssel", OP_ACCUM: "accum",
            OP_CODE_LOOKUP: "clk", OP_CODE_RUNS: "crun", OP_ADAM_GROUPS: "adamg", OP_EVAL_GROUPS: "evg",
            OP_MEL_TILE: "mtile", OP_CODE_STITCH: "cstitch", OP_CODE_TILE: "ctile", OP_COND_STITCH: "cndst",
            OP_WAV_TILE: "wtile", OP_NLL_STITCH: "nllst", OP_SCORE_REDUCE: "sred", OP_SEQ_ALIGN: "align",
            OP_FRAME_STITCH: "fstitch", OP_CODE_SEGMENT: "cseg", OP_SEQ_SEARCH: "search",
            OP_ABX_COUNT: "abx", OP_SEQ_DISCOVER: "discover"}



def uw_chunks(offs, lens):
    """(chunk table as a ctypes array of UwChunk, [first chunk of each tensor] + [number of chunks]) for tensors at flat
    offsets `offs` with `lens` elements: aew_uw_chunks, the arithmetic the tracked Adam launch relies on."""
    lib = load()
    P = len(offs)
    o, ln = (C.c_int64 * P)(*offs), (C.c_int64 * P)(*lens)
    nc, first = C.c_int64(), (C.c_int32 * (P + 1))()
    check(lib.aew_uw_chunks(o, ln, P, None, 0, C.byref(nc), None), "aew_uw_chunks")
    chunks = (UwChunk * max(nc.value, 1))()
    check(lib.aew_uw_chunks(o, ln, P, C.cast(chunks, C.c_void_p), nc.value, C.byref(nc), first), "aew_uw_chunks")
    return chunks, list(first)


def adam_tensor_records(groups, n_tensors: int) -> bytes:
    """The bytes of n_tensors aew_adam_tensor_t records for groups = [(lr, weight_decay, frozen)]: lr rounded to fp32,
    decay = 1 - lr * weight_decay computed in double and rounded to fp32 once (include/aewavenet.h)."""
    import numpy as np
    if len(groups) != n_tensors:
        raise ValueError(f"groups has {len(groups)} records, the flat buffer {n_tensors} tensors")
    lr = np.array([g[0] for g in groups], np.float64)
    wd = np.array([g[1] for g in groups], np.float64)
    if not (np.isfinite(lr).all() and np.isfinite(wd).all() and (lr >= 0).all() and (wd >= 0).all()):
        raise ValueError("groups: lr and weight_decay must be finite and not negative")
    rec = np.zeros(n_tensors, np.dtype([("lr", "<f4"), ("decay", "<f4"), ("frozen", "<i4"), ("pad_", "<i4")]))
    rec["lr"], rec["decay"] = lr, 1.0 - lr * wd
    rec["frozen"] = [1 if g[2] else 0 for g in groups]
    return rec.tobytes()


def select_key(bits: int) -> int:
    """The order key AEW_OP_SEG_SELECT ranks the fp32 value with bit pattern `bits` by: aew_select_key, the kernels' own."""
    key = C.c_uint32()
    check(load().aew_select_key(bits & 0xFFFFFFFF, C.byref(key)), "aew_select_key")
    return key.value


# ---- autoregressive sampler (aew_actor_t / aew_sampler_t) ----
ACT_NONE, ACT_EARLY, ACT_LATE, ACT_RES, ACT_SKIP, ACT_POST1, ACT_POST2, ACT_SAMPLE = -1, 0, 1, 2, 3, 4, 5, 6


class Sbuf(C.Structure):
    _fields_ = [("ptr", vp), ("bstride", i64), ("entry", i64), ("pitch", i64), ("ring", i32), ("layout", i32)]


class Wait(C.Structure):
    _fields_ = [("flags", vp), ("n", i32), ("lag", i32)]


class Actor(C.Structure):
    _fields_ = [("role", i32), ("layer", i32), ("index", i32), ("nt", i32), ("nk", i32), ("nk2", i32),
                ("dil", i32), ("pad", i32), ("wait", Wait * 2), ("flag", vp), ("w", vp), ("w2", vp),
                ("bias", vp), ("bias_pitch", i64), ("in0", Sbuf), ("in1", Sbuf), ("out", Sbuf), ("out2", Sbuf),
                ("n_quant", i32), ("row_bytes", i32)]


class Sampler(C.Structure):
    _fields_ = [("actors", vp), ("n_slots", i32), ("n_batches", i32), ("n_steps", i32), ("flag_stride", i32),
                ("kr_max", i32), ("spin_max", i32), ("flags", vp), ("status", vp), ("forced", vp),
                ("wav_out", vp), ("seed", C.c_uint64), ("nap_eighths", i32), ("pad", i32), ("prof", vp), ("draw", vp)]


class DrawRec(C.Structure):                                # aew_draw_t: the draw controls of one stream
    _fields_ = [("inv_temp", C.c_float), ("top_k", i32), ("top_p", C.c_float), ("flags", i32)]


DRAW_GREEDY = 1                                            # aew_draw_t.flags bit 0


LIB_PATH = os.environ.get("AEW_LIB_PATH") or \
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libaewavenet_hip.so")   # (AEW_LIB_PATH: tools-only builds)
_lib = None


class AewError(RuntimeError):
    pass


def load():
    """Load libaewavenet_hip.so (built by __graft_entry__.build()).  Raises if it is missing
    or if the struct mirrors above have drifted from the header."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64 (same SONAME as /opt/rocm's, which this
    # library is linked against).  Whichever is loaded first serves both, and torch does not find its devices
    # through the system copy ("no ROCm-capable device"), so torch has to be imported before the dlopen below.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise AewError(f"HIP extension not built: {LIB_PATH} is missing "
                       "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                       "There is no CPU fallback for the product path.")
    if torch.cuda.is_available():
        arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
        if arch and not arch.startswith("gfx950"):
            raise AewError(f"libaewavenet_hip.so is built for gfx950 (MI355X) only; device 0 is {arch}")
    lib = C.CDLL(LIB_PATH)
    lib.aew_strerror.restype = C.c_char_p
    lib.aew_run_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.aew_timing_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.aew_selftest.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.aew_tn_slabs.argtypes = [C.c_void_p]
    lib.aew_tn_fold.argtypes = [C.c_void_p]
    lib.aew_tn_group_check.argtypes = [C.c_void_p]
    lib.aew_tn_group_tiles.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aew_nt_kernel.argtypes = [C.c_void_p]
    lib.aew_nt_pick.argtypes = lib.aew_tn_pick.argtypes = lib.aew_tn_group_pick.argtypes = [C.c_void_p, C.c_void_p]
    lib.aew_lc_scatter_needs_zero.argtypes = [C.c_int]
    lib.aew_graph_capture.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    lib.aew_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    lib.aew_graph_destroy.argtypes = [C.c_void_p]
    lib.aew_sampler_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.aew_run_plan_tuned.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    lib.aew_graph_capture_tuned.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]
    for fn in (lib.aew_tuning_default, lib.aew_tuning_get, lib.aew_tuning_set):
        fn.argtypes = [C.c_void_p]
    lib.aew_nt_chain_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.c_int]
    lib.aew_nt_chain_build_tuned.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.c_int, C.c_void_p]
    lib.aew_nt_chain_build_bm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p]
    lib.aew_probe_box.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.aew_nt_chain_dep_tiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.aew_gemm_nt_small_split.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    lib.aew_colsum_det_size.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.aew_grad_norm_size.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.aew_corpus_locate.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.aew_utterance_locate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.aew_segment_ws_bytes.argtypes = [C.c_int64, C.c_int, C.POINTER(C.c_int64)]
    lib.aew_segment_host.argtypes = [C.c_void_p]
    lib.aew_abx_host.argtypes = [C.c_void_p]
    lib.aew_seg_select_size.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.aew_select_key.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
    lib.aew_uw_chunks.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_int64,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    for which, cls in ((0, Op), (1, GemmNT), (2, GemmTN), (3, Seg), (4, View), (5, CopyRec), (6, Actor), (7, Sampler), (8, Tuning),
                       (9, NtStage), (10, NtChain), (11, Adam), (12, GradNorm), (13, UwChunk), (14, UwTrack),
                       (15, UpdateRatio), (16, NtPick), (17, Swap), (18, VqRestart), (19, TnPick), (20, EvalAcc),
                       (21, WindowGather), (22, GradWelford), (23, SegSelect), (25, Accum), (27, CodeLookup), (28, CodeRuns),
                       (29, AdamTensor), (30, AdamGroups), (31, AdamGrouped), (32, EvalGroups), (34, UttRow), (35, MelTile),
                       (36, CodeStitch), (37, CondRow), (38, CodeTile), (39, CondStitch), (41, DrawRec), (42, ScoreRow), (43, WavTile),
                       (44, NllStitch), (45, ScoreReduce), (47, AlignSeq), (48, AlignPair), (49, SeqAlign),
                       (51, SegUtt), (52, FrameStitch), (53, CodeSegment), (55, SearchPair), (56, SeqSearch),
                       (58, AbxGroup), (59, AbxCount), (61, DiscoverPair), (62, SeqDiscover)):
        want = lib.aew_sizeof(which)
        if want != C.sizeof(cls):
            raise AewError(f"ABI mirror drift: sizeof({cls.__name__}) = {C.sizeof(cls)} in Python, "
                           f"{want} in the library")
    if lib.aew_abi_version() != 28:            # (held at 28; the appended records are checked through aew_sizeof above)
        raise AewError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what="aew call", fail_index=None):
    if rc != 0:
        msg = load().aew_strerror(rc).decode()
        at = f" at op {fail_index}" if fail_index is not None else ""
        raise AewError(f"{what} failed{at}: rc={rc} ({msg})")


def default_tuning(**over) -> "Tuning":
    """The library's default tuning record, with fields overridden by keyword."""
    t = Tuning()
    check(load().aew_tuning_default(C.byref(t)), "aew_tuning_default")
    for k, v in over.items():
        if not hasattr(t, k):
            raise AttributeError(f"aew_tuning_t has no field {k}")
        setattr(t, k, int(v))
    return t


def current_tuning(**over) -> "Tuning":
    """A copy of the process-wide tuning record (what the aew_set_* switches have made of it), fields overridden by keyword."""
    t = Tuning()
    check(load().aew_tuning_get(C.byref(t)), "aew_tuning_get")
    for k, v in over.items():
        if not hasattr(t, k):
            raise AttributeError(f"aew_tuning_t has no field {k}")
        setattr(t, k, int(v))
    return t


def tn_slabs(tn: GemmTN) -> int:
    """Number of fp32 partial slabs a TN op writes (host-side mirror is the library itself so
    the split heuristic has a single definition)."""
    return load().aew_tn_slabs(C.byref(tn))


EXPORTS = ("aew_abi_version", "aew_sizeof", "aew_run_plan", "aew_timing_enable",
           "aew_timing_read", "aew_strerror", "aew_selftest", "aew_tn_slabs", "aew_set_tn_safe",
           "aew_graph_capture", "aew_graph_launch", "aew_graph_destroy", "aew_tn_fold", "aew_set_tn_fold_rows",
           "aew_set_lanes", "aew_set_tn_cursor", "aew_set_nt_wave_rows", "aew_set_nt_pipe",
           "aew_set_tn_target_blocks", "aew_set_tn_small", "aew_set_nt_small_tiles", "aew_set_nt_small_deep", "aew_set_nt_small_waves", "aew_set_nf_deep", "aew_set_nf_loaders", "aew_set_nt_rows192",
           "aew_sampler_run", "aew_set_fn", "aew_nt_kernel", "aew_set_tn_big", "aew_set_nt_window", "aew_set_nt_epi_lines", "aew_set_fn_ring3", "aew_set_nt_small_n64", "aew_tn_group_check", "aew_set_nt_mem128", "aew_set_nt_deep", "aew_tuning_default", "aew_tuning_get",
           "aew_tuning_set", "aew_run_plan_tuned", "aew_graph_capture_tuned", "aew_nt_chain_build", "aew_nt_chain_dep_tiles", "aew_probe_box", "aew_gemm_nt_small_split", "aew_colsum_det_size", "aew_nt_chain_build_tuned", "aew_nt_chain_build_bm",
           "aew_grad_norm_size", "aew_uw_chunks", "aew_nt_pick", "aew_lc_scatter_needs_zero", "aew_tn_pick", "aew_tn_group_pick", "aew_tn_group_tiles",
           "aew_corpus_locate", "aew_seg_select_size", "aew_select_key", "aew_utterance_locate",
           "aew_segment_ws_bytes", "aew_segment_host", "aew_abx_host")
