/* aewavenet.h — C ABI of the MI355X-native WaveNet-autoencoder training hot path.
 *
 * The reference (hrbigelow/ae-wavenet) is pure Python on torch ATen; it has no FFI.  Its
 * drop-in boundary is the nn.Module surface (autoencoder_model.py:206-259,
 * mfcc_inverter.py:89-108, driven by chassis.py:151-171).  This header is the C ABI the
 * build adds *underneath* that surface: plain pointers, sizes and POD descriptors, no torch
 * types.  Each entry point / op lists the reference ATen call sites it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative AEW_E_* on argument errors, or a
 *     positive hipError_t; nothing throws across the ABI
 *   - the library never allocates or frees device memory; the caller owns all buffers
 *   - all work is enqueued on the hipStream_t passed in (stream-ordered, no host sync)
 *   - activations are CHANNELS-LAST: tensor[b][t][c], c fastest.  bf16 is stored as uint16
 *   - "row" means a time index t; a buffer is addressed as
 *         ptr + b*batch_stride + row*row_pitch + c            (element units)
 *   - descriptors carry everything an op computes WITH; kernel-shape choices live in a tuning record (aew_tuning_t): the
 *     aew_set_* switches edit the process-wide one, aew_run_plan_tuned takes a caller's own
 *     (kernel shape / schedule choices for A-B measurements and bisecting; results are the same under every setting
 *     unless a switch says otherwise).  They default to the production choice, are not thread-safe, and take effect
 *     for launches / graph captures made afterwards; a caller that never touches them gets a stateless library
 *
 * The hot path is a static LAUNCH PLAN: an array of aew_op_t records executed in order by
 * aew_run_plan().  Almost every record is one of two GEMM forms over *row-affine segments*:
 *
 *   NT ("forward/dgrad"):  C[b][m][n]  = sum_s sum_k A_s[b][m*step_s + off_s][k] * W[n][K_s + k]
 *   TN ("wgrad")        :  dW[b][n][K_s + k] = sum_m G[b][m*gstep + goff][n] * A_s[b][m*step_s + off_s][k]
 *
 * Rows outside a segment's [row_lo,row_hi) read as zero.  With this one form:
 *   dilated causal conv (wavenet.py:100-101)      = 3 segments  x[t], x[t+dil], cond[t+lead]
 *   strided encoder conv (wave_encoder.py:39)      = f segments  x[t*s + tap]
 *   ConvTranspose1d upsampler (wavenet.py:154)     = f/s segments per output phase, x[q - j]
 *   every dgrad                                    = the transposed segment table
 *   every wgrad                                    = TN over the same segments
 */
#ifndef AEWAVENET_H
#define AEWAVENET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The number is held at 28 across the gradient-statistics additions (AEW_OP_GRAD_WELFORD, AEW_OP_SEG_SELECT): they are
 * append-only - two op kinds behind the existing ones, two descriptors that fit the union's size, aew_sizeof indices 22
 * and 23, two host functions; no existing record, op number or function changed - so a caller built against 28 runs
 * unchanged.  A binding that wants the additions finds them through aew_sizeof(22) / aew_sizeof(23) (-1 in a library
 * without them).  Every later addition follows the same rule and is listed at aew_sizeof below (the last: 37 .. 39,
 * aew_cond_row_t, aew_code_tile_t / AEW_OP_CODE_TILE, aew_cond_stitch_t / AEW_OP_COND_STITCH; 41, aew_draw_t, with the
 * `draw` pointer appended to aew_sampler_t - index 40 stays unused, it answers -1; 42 .. 45, aew_score_row_t,
 * aew_wav_tile_t / AEW_OP_WAV_TILE, aew_nll_stitch_t / AEW_OP_NLL_STITCH, aew_score_reduce_t / AEW_OP_SCORE_REDUCE;
 * 47 .. 49, aew_align_seq_t, aew_align_pair_t, aew_seq_align_t / AEW_OP_SEQ_ALIGN - index 46 stays unused; 51 .. 53, aew_seg_utt_t,
 * aew_frame_stitch_t / AEW_OP_FRAME_STITCH, aew_code_segment_t / AEW_OP_CODE_SEGMENT - index 50 stays unused; 55 / 56,
 * aew_search_pair_t, aew_seq_search_t / AEW_OP_SEQ_SEARCH - index 54 stays unused; 58 / 59, aew_abx_group_t,
 * aew_abx_count_t / AEW_OP_ABX_COUNT with the host function aew_abx_host - index 57 stays unused; 61 / 62,
 * aew_discover_pair_t, aew_seq_discover_t / AEW_OP_SEQ_DISCOVER - index 60 stays unused.  The number does NOT
 * move for AEW_OP_SEQ_DISCOVER either: one op kind behind the last, a descriptor inside the union's size, no existing
 * record, op number or function changed). */
#define AEW_ABI_VERSION 28
#define AEW_MAX_SEGS 32

/* error codes (negative; positive values are hipError_t) */
#define AEW_E_ARG      (-1)   /* malformed descriptor */
#define AEW_E_UNSUP    (-2)   /* unsupported op / dtype / flag combination */
#define AEW_E_ALIGN    (-3)   /* pointer or pitch violates the documented alignment */

/* element types */
#define AEW_BF16 0
#define AEW_F32  1

/* ---------------------------------------------------------------------------------------
 * A-operand segment: rows m*row_step + row_off of a channels-last buffer, k_len channels.
 * k_len must be a multiple of the kernel's K tile (64 for bf16, 32 for f32); the buffer
 * must hold k_len (zero-padded) channels per row.  16-byte alignment of ptr and of
 * row_pitch*sizeof(elem) is required.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const void* ptr;
    int64_t batch_stride;
    int32_t row_pitch;
    int32_t row_step;
    int32_t row_off;
    int32_t row_lo, row_hi;      /* valid source rows [lo,hi); others read as zero */
    int32_t k_len;
} aew_seg_t;

/* generic channels-last view used by epilogues */
typedef struct {
    void* ptr;
    int64_t batch_stride;
    int32_t row_pitch;
    int32_t row_step;            /* view row = m*row_step + row_off */
    int32_t row_off;
    int32_t row_lo, row_hi;      /* rows of the *view* that exist: stores outside are dropped,
                                    loads outside read as zero */
    int32_t dtype;               /* AEW_BF16 | AEW_F32 */
} aew_view_t;

/* NT epilogues */
#define AEW_EPI_STORE     0   /* flag-driven store, see AEW_EF_* */
#define AEW_EPI_GATED     1   /* a=tanh(f+bf), s=sigmoid(g+bg); N is (16 filt | 16 gate)-interleaved.
                                 out0 = z = a*s, out1 = dz/df = s(1-a^2), out2 = dz/dg = a s(1-s)
                                 (bf16)                                   wavenet.py:100-102 */
#define AEW_EPI_RES_SKIP  2   /* n<n_split: out0[m]=acc+aux0[m] (residual, wavenet.py:108-109)
                                 n>=n_split: out1[m][n-n_split] (+)= acc (skip sum, :103,:357);
                                 with AEW_EF_OUT2_RELU also out2=relu(out1) bf16 (:359)          */
#define AEW_EPI_DFG       3   /* acc=dz; aux0=dz/df, aux1=dz/dg (from GATED); out0 = (dfilt|dgate)-
                                 interleaved bf16: dz*aux0, dz*aux1    (backward of wavenet.py:102) */

/* AEW_EPI_STORE flags */
#define AEW_EF_BIAS        (1u << 0)  /* val += bias[b*bias_bs + n]                           */
#define AEW_EF_RELU        (1u << 1)  /* val = max(val,0)          (after bias)               */
#define AEW_EF_OUT1_PRE    (1u << 2)  /* out1 = val  (before the aux add; encoder relu out)    */
#define AEW_EF_ADD_AUX0    (1u << 3)  /* val += aux0[view row of m][n]  (zero outside range)   */
#define AEW_EF_MUL_POS1    (1u << 4)  /* val *= (aux1[m][n] > 0)                               */
#define AEW_EF_OUT1_POS1   (1u << 5)  /* out1 = val * (aux1[m][n] > 0)  (out0 keeps val)       */
#define AEW_EF_ACCUM       (1u << 6)  /* RES_SKIP: out1 += acc instead of =                    */
#define AEW_EF_OUT2_RELU   (1u << 7)  /* RES_SKIP: out2 = relu(new out1) as bf16              */
#define AEW_EF_RELU_POST   (1u << 9)  /* val = max(val,0) AFTER the aux0 add (sum of partial GEMMs, then relu) */
#define AEW_EF_OUT2_COPY   (1u << 10) /* out2 = the value stored to out0, in out2's dtype (bf16 copy of an fp32
                                         activation for the bf16 backward GEMMs)                */
#define AEW_EF_COUNT_ZERO  (1u << 8)  /* atomically add #(out0==0) into counter (enc_az metric,
                                         wave_encoder.py:46)                                   */

typedef struct {
    int32_t dtype;               /* operand type AEW_BF16 | AEW_F32 */
    int32_t impl;                /* 0 = tiled MFMA kernel, 1 = scalar check kernel, 2 = full-N MFMA kernel with
                                    loader / consumer waves (aew_fn.hip; falls back to 0 when the shape is not
                                    covered).  Same results bit for bit                            */
    int32_t M;                   /* output rows per batch                                     */
    int32_t N;                   /* output columns to store: multiple of 8 (bf16) / 4 (f32)   */
    int32_t N_pad;               /* rows of W (multiple of 128 for bf16, 64 for f32)          */
    int32_t batch;
    int32_t n_segs;
    int32_t K_total;             /* sum of k_len = row length of W                            */
    aew_seg_t seg[AEW_MAX_SEGS];
    const void* W;               /* packed [N_pad][K_total], same dtype as the operands       */
    int32_t epi;
    uint32_t flags;
    aew_view_t out0, out1, out2; /* views are indexed with the GEMM row m                     */
    aew_view_t aux0, aux1;
    const float* bias;           /* fp32 [*, N_pad]                                           */
    int64_t bias_bs;             /* per-batch stride of bias (0 = shared)                     */
    int32_t n_split;             /* RES_SKIP column boundary (multiple of the N tile)         */
    int32_t reserved;
    unsigned long long* counter; /* AEW_EF_COUNT_ZERO target                                  */
    /* Fused gated layer (AEW_EPI_GATED only; wavenet.py:100-109).  With W2 != NULL the op also computes the
     * residual 1x1 of the layer from the z tile it has just produced:
     *     out3[b][m][n2] = sum_k z[b][m][k] * W2[n2][k] + aux0[b][m][n2]        n2 < N2, k < N_pad / 2
     * (z = the bf16 values written to out0, so the result equals GATED followed by a STORE | ADD_AUX0 GEMM over
     * out0; impl 0 / 1 execute it exactly that way, impl 2 keeps the z tile in LDS).                        */
    const void* W2;              /* packed [N2_pad][N_pad / 2] bf16                                          */
    int32_t N2, N2_pad;          /* N2 multiple of 8, N2_pad multiple of 128                                 */
    aew_view_t out3;
    /* Split-K of the exact fp32 kernel (ABI 19; AEW_F32, impl 0, AEW_EPI_STORE only; wave_encoder.py:39, vqema_bn.py:131).
     * k_split = S in {2, 4}: the concatenated K axis is cut into S contiguous ranges of K_total / S channels (a multiple of
     * 32), each a k-ascending fmaf chain of its own on its own workgroup; the partial sums meet in the FIXED order
     *     S = 2: p0 + p1          S = 4: (p0 + p1) + (p2 + p3)         (plain fp32 adds, then bias / relu / ...)
     * whichever workgroup arrives last does the combine and the epilogue - the order of arrival does not enter the result.
     * This IS the canonical summation order of the op (oracle/exact_chain.c: aewo_conv_cl ksplit), chosen so that the
     * 180-block launches of the encoder (232-560 rows in all) become 720 blocks with a quarter of the serial K loop each.
     * ksplit_ws: device fp32 [S][rows_pad][N_pad], rows_pad = M * batch rounded up to 32; ksplit_tickets: device uint32
     * [tiles of 16 rows x 16 channels rounded up], ZERO before the first launch (the combine resets them).  0 / 1 = off.
     *
     * AEW_BF16, impl 0: a HINT for launches of very few workgroups - the upsampler / encoder data gradients,
     * 16-112 blocks of 64 x 64 on 256 CUs, each a lone block's LDS fill latency long (wavenet.py:275, wave_encoder.py:39
     * backward).  k_split = S in 2..8 with K_total a multiple of 64 * S: the launch becomes S copies of its tile grid, copy s
     * contracting K tiles [s, s + 1) * K_total / 64 / S; the partial accumulators meet in ascending order of s (a fixed
     * order: results are deterministic, but NOT those of the unsplit launch - bf16 operands, fp32 accumulation, the same
     * tolerance class) in the workgroup that arrives last.  Honoured only where the launcher takes its 64 x 64 shape under
     * the tuning record in force (else the whole K axis is contracted by one workgroup, the slabs stay unused);
     * aew_gemm_nt_small_split() states the rule and the sizes: ksplit_ws = ws_bytes bytes (16-byte aligned),
     * ksplit_tickets = n_tickets uint32, zero before the first launch.                                                   */
    int32_t k_split;
    int32_t pad2_;
    float* ksplit_ws;
    uint32_t* ksplit_tickets;
} aew_gemm_nt_t;

typedef struct {
    int32_t dtype;
    int32_t impl;
    int32_t Mc;                  /* contraction rows per batch                                */
    int32_t batch;
    int32_t N;                   /* real columns of G                                         */
    int32_t N_pad;               /* multiple of the tile (128 bf16 / 64 f32); G has N_pad cols */
    aew_seg_t g;                 /* G operand; k_len ignored                                  */
    int32_t n_segs;
    int32_t K_total;
    aew_seg_t seg[AEW_MAX_SEGS];
    float* out;                  /* fp32 [batch][N_pad][K_total] per-batch partial sums       */
    int64_t out_batch_stride;
    /* Grouped form only (AEW_OP_GEMM_TN_GROUP: the contraction runs over the batch elements in order inside one
     * block).  With snap_out != NULL the running column sum_{b' <= b} sum_m G[b'][m][n] * A[b'][m][snap_k] is
     * written after every batch element b:  snap_out[b * snap_bs + n].  With a constant-one channel at snap_k
     * (the pad channel R of x, aew_base_gather_t.ones_channel) that is the running column sum of G - the per-batch
     * bias / speaker-embedding gradients come out of the weight-gradient GEMM for free (aew_spk_bwd_t.colsum_running). */
    float* snap_out;
    int64_t snap_bs;
    int32_t snap_k;              /* column of the concatenated K axis; -1 (with snap_out): no A column - the running
                                    column sums of G themselves, from an all-ones MFMA operand in the blocks of the
                                    first k tile (layers without a spare pad channel for the ones: R a multiple of 128) */
    int32_t pad_;
    /* Grouped form only.  colsum_out != NULL: colsum_out[n] = sum_b sum_m G[b][m][n] for n < N - the bias gradient of
     * the layer whose weight gradient this is (its G operand is the gradient of the layer's pre-activation) - written
     * by the blocks of the first k tile from an extra all-ones MFMA operand: no separate column-sum launch, one
     * summation order (deterministic, no atomics).                                                                  */
    float* colsum_out;
    /* Grouped form only.  grp_splits > 0: the contraction is cut like a stand-alone TN op's - one block per (output
     * tile, batch element, chunk of grp_rows rows), grp_splits chunks per batch element, partial sums to slab
     * b * grp_splits + chunk of `out` (out_batch_stride apart; the unpack sums them).  For matrices with few output
     * tiles and a long contraction (the upsampler weights), where one block per tile would be a lone latency-bound
     * chain.  snap_out / colsum_out need grp_splits = 0 (one block sees every row).                              */
    int32_t grp_splits, grp_rows;
} aew_gemm_tn_t;

/* ---------------------------------------------------------------------------------------
 * Grouped weight gradients: the output tiles of SEVERAL TN descriptors as one launch, each tile contracting over
 * the WHOLE time axis and all batch elements (k ascending, b ascending) in one block.  One fp32 result per
 * descriptor (desc.out[N_pad][K_total], no split-K slabs to write and sum), and enough tiles to fill the chip
 * without splitting (20 layers x (4 x 7 + 3 x 2) tiles in the decoder).  Descriptors and the tile map live in
 * DEVICE memory (built once per plan).  tile_map[p] = desc << 22 | chunk << 12 | tile (tile = nt * (K_total / 128) + kt;
 * chunk = 0 unless the descriptor is split, see aew_gemm_tn_t.grp_splits), or -1: block p idles.  Workgroup p runs on XCD p % 8, so the builder places tiles that share operands on one XCD.
 * bf16 only.  Same products as aew_gemm_tn_t ops; the summation order differs (one chain instead of slabs).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const aew_gemm_tn_t* descs;  /* device                                                      */
    const int32_t* tile_map;     /* device                                                      */
    int32_t n_descs, n_blocks;
    int32_t tile;                /* 128: 128 x 128 output tiles, 4 waves, three blocks per CU
                                    256: 256 x 256 tiles (half the operand bytes staged per FLOP), 8 waves, one block
                                         per CU; tile = nt * ((K_total / 128 + 1) / 2) + kt in 256-column units, halves
                                         beyond N_pad / K_total are skipped
                                    384 (ABI 20): EIGHT waves of 64 x 64 on a 128 (k) x 256 (n) tile - or 256 (k) x 128 (n)
                                         where K_total is a multiple of 256 and N_pad is not - two blocks per CU on a
                                         3 x 24 KiB ring (the NT kernels' shape: 1.5 x the MFMAs per staged byte of the
                                         128-tile, four waves per SIMD); tile = nt * nkt + kt in that grid (aew_tn_group_tiles);
                                         no split descriptors (grp_splits = 0), no cursor; results bit-identical to tile = 128 */
    int32_t cursor_stride;       /* words per descriptor in `cursors` (>= 64)                                          */
    /* Optional row cursor (ABI 18; tile = 128 only; non-NULL = pace this launch): device
     * [n_descs][cursor_stride] uint32, ZERO before every launch (epoch / slack: aew_set_tn_cursor); word i of a descriptor's row = the epoch tile i is
     * about to issue.  The output tiles of one descriptor share their operand columns; the cursor keeps them within
     * `slack` epochs (of `epoch` 32-row stages) of each other as they walk down the rows, so that what one tile
     * fetched is still in its XCD's L2 when its siblings read it.  Performance only: a tile whose wait times out (a
     * sibling not resident, or on another XCD) runs free from there on; descriptors with > 64 tiles are not paced.
     * NULL = off.                                                                                                    */
    uint32_t* cursors;
} aew_gemm_tn_group_t;

/* ---------------------------------------------------------------------------------------
 * table-driven strided copy / convert / reduce (weight pack, gradient unpack, NCL<->NLC)
 *   dst[sum_d i_d*ds_d] = cvt( sum_{r<red_n} src[sum_d i_d*ss_d + r*red_stride] )
 * Tiled form (tr_a > 0; red_n = 1, no accumulate, f32 source): dims[3] is the dim the SOURCE is (nearly) contiguous in,
 * dims[2] the one the DESTINATION is contiguous in (ds[2] = 1); a block moves one tr_a x tr_b tile of that plane through
 * LDS, reading along dims[3] and writing along dims[2] (transposing weight packs: both sides coalesced).  Same result
 * as the element-wise forms.  Blocks per record: dims[0] * dims[1] * ceil(dims[2] / tr_b) * ceil(dims[3] / tr_a).
 * Interleave forms (tr_a = -k, k = 2..4 taps of a conv weight; f32 source, red_n = 1, no accumulate, 16-byte aligned):
 *   tr_b = 1  [..][k][c] -> [..][c][k]:  dims[2] = k, dims[3] = c (ss[3] = 1, ds[2] = 1, ds[3] = k), f32 destination
 *   tr_b = 2  [..][c][k] -> [..][k][c]:  dims[2] = c, dims[3] = k (ss[3] = 1, ss[2] = k, ds[2] = 1), f32 or bf16
 * a thread permutes W = 4 (8 for bf16) channels of all taps in registers; blocks: ceil(dims[0] * dims[1] * c / W / 256).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const void* src;
    void* dst;
    int32_t dims[4];
    int64_t ss[4], ds[4];
    int32_t src_dtype, dst_dtype;
    int32_t red_n;
    int32_t accumulate;          /* dst += (f32 dst only) */
    int64_t red_stride;
    float scale;
    int32_t first_block;         /* filled by the host: first block of this record (1024 elements per block, or one
                                    tile in the tiled form)                                                       */
    int32_t tr_a, tr_b;          /* tr_a > 0: tiled form, tile extents along dims[3] / dims[2] (tr_a * tr_b <= 4096,
                                    tr_b * (tr_a | 1) <= 4160); tr_a < 0: interleave forms; 0 = element-wise      */
} aew_copy_rec_t;

typedef struct {
    const aew_copy_rec_t* recs;  /* DEVICE array                                              */
    const int32_t* block_rec;    /* DEVICE array: record index of every block                 */
    int32_t n_blocks;
    int32_t n_recs;
} aew_copy_table_t;

/* ---------------------------------------------------------------------------------------
 * small ops
 * ------------------------------------------------------------------------------------- */
typedef struct {                 /* nearest code  (vqema_bn.py:135-142, vq_bn.py:39-41)        */
    const float* ze;             /* [Q][d_pitch] fp32, Q = B*N_e                              */
    const float* emb;            /* [K][d]                                                    */
    int32_t Q, K, d, d_pitch;
    int32_t metric;              /* 0 scaled_l2, 1 sq_l2                                      */
    int64_t* ind;                /* [Q]                                                       */
    float* dist;                 /* [Q]                                                       */
    float* zq;                   /* [Q][d_pitch] (pad channels zeroed)                        */
    void* scratch; int32_t n_split;   /* optional: 8*Q*n_split bytes.  The K codes are then scanned by n_split
                                         blocks per query (partial minima into scratch) and a second tiny kernel
                                         combines them in ascending split order: same result bit for bit, 4x
                                         shorter critical path at Q = 232, K = 4096                           */
} aew_vq_nearest_t;

typedef struct {                 /* z_sum/n_sum, deterministic order (vqema_bn.py:172-188)     */
    const float* ze; const int64_t* ind;
    int32_t Q, K, d, d_pitch;
    float* z_sum; float* n_sum;  /* [K][d], [K]                                               */
    float* hist;                 /* optional ind_hist accumulator [K] (util.py:107-123)       */
} aew_vq_stats_t;

typedef struct {                 /* EMA + optional codebook refresh (vqema_bn.py:190-195,216) */
    float* numer; float* denom; const float* z_sum; const float* n_sum;
    float* emb;                  /* written when update_codebook != 0; 2 = only rows with denom > 0 (with
                                    gamma = 0, gamma_comp = 1 that is the centroid step of Lloyd's k-means,
                                    autoencoder_model.py:171-199)                              */
    int32_t K, d, update_codebook;
    float gamma, gamma_comp;
    const uint32_t* guard;       /* ABI 20, optional: device word; non-zero = the op does nothing (see aew_adam_t.guard) */
} aew_vq_ema_t;

/* Restart dead codebook entries from this step's encoder outputs (ABI 25; VQ-VAE-EMA only).  One workgroup of 1024
 * threads, so every order is fixed; no atomics.
 *   dead list : D = every k in [0, K) with !(denom[k] >= min_usage), ascending (a NaN denominator is dead);
 *               n_dead = |D|, n = min(n_dead, Q, max_codes); only D[0 .. n) are restarted.
 *   rows      : h = mix64(mix64(seed + G) ^ (call + G)), G = 0x9e3779b97f4a7c15 and mix64 the splitmix64 finaliser of
 *               aew_jitter_t; a = mix64(h ^ 1) % Q; Q == 1: b = 1; otherwise b0 = mix64(h ^ 2) % (Q - 1) and b is the
 *               first c_i = 1 + (b0 + i) % (Q - 1), i = 0, 1, ..., with gcd(c_i, Q) == 1 (c = 1 qualifies, so it ends).
 *               Restart r takes row q_r = (a + r * b) % Q in 64-bit arithmetic: b is coprime to Q, so the n rows are
 *               distinct - no two codes are seeded with the same vector.
 *   writes    : numer[k][j] = __fmul_rn(ze[q][j], denom_init), emb[k][j] = __fdiv_rn(numer[k][j], denom_init) - the
 *               expression of aew_vq_ema_t's codebook refresh, which therefore reproduces emb bit for bit - and
 *               denom[k] = denom_init, for j < d.  denom_init = 1 makes the code the encoder output exactly.  Nothing
 *               else in the three buffers changes.
 * AEW_E_ARG: Q, K or d < 1, d_pitch < d, max_codes outside 1 .. AEW_VQ_RESTART_MAX, denom_init not finite or <= 0,
 * min_usage NaN, a NULL ze / emb / numer / denom / out; AEW_E_ALIGN: a pointer that is not 4-byte aligned.  Both before
 * any launch. */
#define AEW_VQ_RESTART_MAX 1024
typedef struct {
    const float* ze; int32_t Q, d, d_pitch;   /* this step's encoder outputs [Q][d_pitch] (bn.lin)            */
    float* emb; float* numer; float* denom;   /* [K][d], [K][d], [K]                                          */
    int32_t K;
    int32_t max_codes;                        /* 1 .. AEW_VQ_RESTART_MAX (1024): at most this many per launch  */
    float min_usage;                          /* code k is dead iff !(denom[k] >= min_usage)  (NaN counts)     */
    float denom_init;                         /* > 0, finite: the denominator a restarted code gets            */
    uint64_t seed, call;                      /* counter-based choice of the rows: no state between launches   */
    int32_t* out;                             /* [4]: dead codes found, codes restarted, running total of
                                                 restarted codes (zeroed by the caller once), 0                */
    int32_t* pairs;                           /* optional [max_codes][2]: (k, q) of each restart, r ascending;
                                                 rows >= out[1] are written as (-1, -1)                        */
    const uint32_t* guard;                    /* optional, like aew_vq_ema_t.guard: non-zero = nothing is written */
} aew_vq_restart_t;

typedef struct {                 /* d(ze) = d(zq) + gscale*gamma * d(min_dist)/d(ze)          */
    const float* ze; const float* emb; const int64_t* ind; const float* dzq;
    int32_t Q, d, d_pitch, metric;
    float coef;                  /* vq_gamma * upstream loss gradient                         */
    float demb_coef;             /* upstream loss gradient (weight of the l2 term, vq_bn.py:78) */
    float* dze;                  /* [Q][d_pitch]                                              */
    float* demb;                 /* optional [K][d], pre-zeroed: d/d(emb) of sum (sg(ze)-emb)^2 */
    const float* gmul;           /* optional device scalar: upstream d(L)/d(loss) of THIS backward call; multiplies
                                    coef and demb_coef at run time (a captured graph stays valid for any value)  */
} aew_vq_bwd_t;

typedef struct {                 /* jitter gather (wavenet.py:330-336) fp32 -> bf16           */
    const float* src; int64_t src_bs; int32_t src_pitch;   /* [B][N][C]                       */
    const int64_t* jitter; int32_t jit_pitch;              /* [B][N]                          */
    uint16_t* dst; int64_t dst_bs; int32_t dst_pitch;      /* [B][N][C_pad] bf16              */
    int32_t B, N, C, C_pad;
    int32_t take_compat;         /* 1: reproduce torch.take flattening (SURVEY C-1)           */
} aew_lc_gather_t;

typedef struct {                 /* transpose of the gather: dsrc[b][j][c] += d[b][t][c]       */
    const float* d; int64_t d_bs; int32_t d_pitch;
    const int64_t* jitter; int32_t jit_pitch;
    float* dsrc; int64_t dsrc_bs; int32_t dsrc_pitch;
    int32_t B, N, C;
    int32_t take_compat;
} aew_lc_scatter_t;
/* 1: an AEW_OP_LC_SCATTER over n conditioning vectors ADDS into dsrc (atomics: the plan zeroes dsrc in front of it);
 * 0: it runs in its gather form, which writes every element of dsrc[b][j][0:C] (no zeroing needed).  Host-only. */
int aew_lc_scatter_needs_zero(int n);

typedef struct {                 /* per-(batch,layer) gated bias incl. speaker term           */
    /* bias[b][l][pack(co)] = conv_bias_l[co] + sum_j V_l[co][C_lc + j] * gc[b][j]
       gc[b] = Wspk[:, voice[b]] + bspk             (wavenet.py:135-139 folded)   */
    const float* params;         /* flat fp32 parameter buffer                                */
    const int64_t* voice;        /* [B]                                                       */
    const int64_t* off_bias_sig; const int64_t* off_bias_gate;  /* DEVICE [L] offsets or -1   */
    const int64_t* off_proj_sig; const int64_t* off_proj_gate;  /* DEVICE [L] offsets         */
    int64_t off_spk_w, off_spk_b;                              /* -1 if no bias               */
    int32_t B, L, D, D_pad, C_lc, G, n_speakers;
    float* bias;                 /* [B][L][2*D_pad]                                           */
    float* gc;                   /* [B][G] saved for backward                                 */
} aew_spk_bias_t;

typedef struct {                 /* backward of the above from per-batch column sums of dfg; G <= 16 (AEW_E_UNSUP beyond: the
                                    kernel holds a projection row in registers).  The batch is cut into chunks of 16
                                    elements.  B <= 16: one chunk, the bias / projection gradients of the op's layers are
                                    plain stores.  B > 16: every chunk ADDS its partial bias / projection sums with fp32
                                    atomics, so the caller zeroes those gradients first; two chunks (B <= 32) add
                                    commutatively and the result is still bit-reproducible, three or more (B > 32) add in
                                    the scheduler's order, WITH OR WITHOUT aew_tuning_t.deterministic              */
    const float* params; const int64_t* voice;
    const int64_t* off_bias_sig; const int64_t* off_bias_gate;
    const int64_t* off_proj_sig; const int64_t* off_proj_gate;
    int64_t off_spk_w, off_spk_b;
    int32_t B, L, D, D_pad, C_lc, G, n_speakers;
    const float* colsum;         /* [B][L][2*D_pad]                                           */
    const float* gc;             /* [B][G]                                                    */
    float* grads;                /* flat fp32 gradient buffer (same offsets as params)        */
    int32_t colsum_running;      /* layers l < colsum_running: colsum[b][l] holds the sum over batch elements 0..b
                                    (aew_gemm_tn_t.snap_out); the per-batch value is colsum[b] - colsum[b-1]  */
    int32_t layer_range;         /* 0: all L layers.  Else first layer | count << 16: this op covers layers [first, first +
                                    count) only (data parallel with two grouped wgrad launches: the upper layers' bias /
                                    projection gradients right after the first group; the speaker-embedding sums of the
                                    parts add up in `grads`)                                                       */
    /* ABI 20, deterministic form (aew_tuning_t.deterministic != 0 and both pointers set): the speaker-embedding sums -
     * one term per (layer, filt | gate) block - go to det_scratch ([count][2][chunks][16][16] floats, count = layers of
     * this op) and the block that draws the last ticket (det_tickets[0]: zeroed once by the caller, left zero by every
     * launch) adds them layer ascending, filt before gate, batch element ascending; without it they are fp32 atomics. */
    float* det_scratch; uint32_t* det_tickets;
} aew_spk_bwd_t;

typedef struct {                 /* base layer as a column gather (wavenet.py:348-351)        */
    const float* wav; int32_t wav_pitch; int32_t wav_off;   /* [B][n_wav] float-encoded ints  */
    const float* W; const float* bias;                      /* [R][Q] (k=1), [R] or NULL      */
    const float* Wt;             /* optional transposed copy [Q][R_pad] (pad columns zero): a row of x
                                    is then ONE contiguous read instead of R strided ones            */
    int32_t B, T, R, R_pad, Q;
    uint16_t* x; int64_t x_bs; int32_t x_pitch;             /* bf16 [B][T][R_pad]             */
    uint16_t* onehot; int64_t oh_bs; int32_t oh_pitch;      /* optional bf16 [B][T][Q_pad]    */
    int32_t Q_pad;
    int32_t ones_channel;        /* 1: write 1.0 into pad channel R (requires R < R_pad).  The padded
                                    weight rows/cols are zero, so the constant propagates through the
                                    residual adds untouched and column R of every gated-layer wgrad
                                    GEMM equals the column sums of dfg (= the gated bias gradients)   */
} aew_base_gather_t;

typedef struct {                 /* fused log-softmax + NLL (+ gradient)  wavenet.py:543-547  */
    const float* logits; int64_t bs; int32_t pitch;         /* fp32 [B][w][Q_pad]             */
    const float* wav; int32_t wav_pitch; int32_t tgt_off;   /* target[b][u] = wav[b][tgt_off+u] */
    int32_t B, w, Q, Q_pad;      /* positions u in [0, w-1) carry loss; u = w-1 is dropped    */
    float* nll;                  /* fwd: [B][w] per-position nll (0 at u=w-1)                 */
    float* ptgt;                 /* fwd: [B][w] probability of the target (chassis.py:266-270)*/
    uint16_t* dlogits; int64_t dl_bs; int32_t dl_pitch;     /* bwd: bf16 [B][w][Q_pad]        */
    float scale;                 /* bwd: d(loss)/d(nll term)                                  */
    int32_t backward;
    const float* gmul;           /* optional device scalar: upstream d(L)/d(loss), multiplies scale at run time */
    float* peak; int32_t* amax;  /* fwd, optional: [B][w] peak log-probability max_c log p(c) and its (lowest) class per
                                    position - what aew_vq_diag_t reduces (vqema_bn.py:261-263) without reading the
                                    logits again.  Set both or neither (AEW_E_ARG).  Only the 256-class register form
                                    writes them: Q == 256, Q_pad == 256, pitch % 4 == 0 and bs % 4 == 0; any other forward
                                    descriptor that sets them is refused with AEW_E_UNSUP before any launch      */
} aew_softmax_nll_t;

typedef struct {                 /* MFCC + delta + delta-delta front-end on the device (mfcc.py:39-76: librosa.feature.mfcc
                                    and librosa.feature.delta on the host in the reference's DataLoader, data.py:230).
                                    Frame f of the call covers y[f*hop - win/2, f*hop + win/2), y = left_pad zeros + wav,
                                    reflected at both ends; |DFT|^2 -> mel -> dB (floor max - 80 over the whole call)
                                    -> DCT-II -> trim -> Savitzky-Golay derivatives (width 9).  Tables come from the host. */
    const float* wav; int64_t wav_bs; int32_t n;            /* [B][n] samples (float-encoded)                  */
    int32_t B, win, hop, n_bins, n_mels, n_mfcc;            /* win <= 1024, n_bins = win/2 + 1, n_mels <= 128, n_mfcc <= 16 */
    int32_t left_pad, trim_left, trim_right, n_frames;      /* n_frames = 1 + (left_pad + n) / hop, before trimming */
    const float* window;         /* [win]                                                      */
    const float* twiddle;        /* [win][2]  cos, sin (2 pi j / win)                          */
    const float* melw;           /* [n_mels][n_bins]                                           */
    const float* dct;            /* [n_mfcc][n_mels]                                           */
    const float* sg;             /* [2][81]: per derivative 9 interior taps, 4x9 left-edge and 4x9 right-edge rows */
    float* scratch;              /* B * n_frames * (n_mels + 1 + n_mfcc) floats                */
    float* out; int64_t out_bs; int32_t out_pitch;          /* [B][3*n_mfcc][out_pitch]; frames n_frames - trims (>= 9) */
} aew_mfcc_t;

typedef struct {                 /* per-step diagnostics of the reference's loss module as fused reductions
                                    (vqema_bn.py:155-160 and :251-264, util.py:98-105; chassis.py:180-185 reads them):
                                    out[0..1] min / max ||ze||, [2..3] min / max ||emb||, [4] entropy (bits) of the
                                    normalised index histogram, [5] codes used this step, [6] mean, [7] unbiased std
                                    of the peak log-probability over the positions that carry loss, [8] number of
                                    distinct arg-max classes.  Groups with a NULL pointer are skipped (zeros).   */
    const float* ze; int32_t Q, d, d_pitch;
    const float* emb; int32_t K;
    const float* hist;           /* accumulated index histogram [K] (aew_vq_stats_t.hist)      */
    const float* n_sum;          /* this step's counts [K]                                     */
    const float* logits; int64_t bs; int32_t pitch;         /* fp32 [B][w][>= n_quant]; u = w-1 is dropped */
    int32_t B, w, n_quant;       /* n_quant <= 256                                             */
    void* scratch;               /* >= 2 KiB, written by the op (per-slice partial results; with `logits` the
                                    class bins).  NULL (not with `logits`): one block does everything            */
    float* out;                  /* [12]                                                       */
    const float* peak; const int32_t* amax;   /* instead of `logits`: the per-position arrays aew_softmax_nll_t wrote
                                                 ([B][w], u = w-1 dropped); out[6..8] come from them               */
} aew_vq_diag_t;

typedef struct {                 /* first two moments of a channels-last view: the gradient statistics run() reports
                                    every step (autoencoder_model.py:252-257 mel_grad_sd / bn_grad_sd,
                                    mfcc_inverter.py:100-106 mel_grad_sd / mel_grad_mean), over x[b][m][0:cols],
                                    b < batch, m < rows.  out[0] mean, out[1] unbiased std (torch.std), out[2] sum,
                                    out[3] sum of squares.  One block, fp64 accumulation in a fixed order.       */
    aew_view_t x; int32_t rows, cols, batch;
    float* out;                  /* [4] */
} aew_moments_t;

typedef struct {                 /* column sums over rows: out[b][n] (+)= sum_m x[b][m][n]     */
    aew_seg_t x; int32_t dtype; int32_t M, N, batch;
    float* out; int64_t out_bs; int32_t accumulate;
    /* ABI 20, deterministic form (aew_tuning_t.deterministic != 0 and both pointers set): the row chunks write their
     * partial sums to det_scratch (aew_colsum_det_size floats) instead of adding atomically; the block that draws the
     * last ticket of its output (det_tickets: zeroed once by the caller, left zero by every launch) adds them in a
     * fixed order - batch element ascending, row chunk ascending - and is the only writer of that output.          */
    int32_t pad_;
    float* det_scratch; uint32_t* det_tickets;
} aew_colsum_t;

typedef struct {                 /* v_i = scale_i * sum(x_i[0:n_i]);  out[1+i] = v_i;
                                    out[0] = sum_i (clamp_i ? post_scale_i*max(v_i, clamp_min_i) : v_i)
                                    (loss scalar; the clamp is SGVB's free-nats, vae_bn.py:113-116) */
    const float* x[4]; int32_t n[4]; float scale[4]; int32_t clamp[4]; float clamp_min[4];
    float post_scale[4]; int32_t n_terms;
    float* out;                  /* [5] */
    const float* post_scale_dev[4];   /* if non-NULL, post_scale_i is read from device memory at run time
                                         (values that change every step, e.g. the KL anneal weight, must not
                                         be frozen into a captured graph)                                    */
} aew_reduce_t;

/* ---------------------------------------------------------------------------------------
 * Evaluation accumulator (ABI 27): folds one evaluated batch into a running record that stays on the device - what a
 * validation loop needs (held-out loss, bits per sample, top-1 accuracy, code perplexity) without a host synchronisation
 * per batch and without touching anything a training step reads.  One launch per batch, ONE workgroup of 1024 threads.
 *
 * finalize == 0 (accumulate).  With P = B * (w - 1) positions that carry loss, i = b * (w - 1) + u (u = w - 1 is dropped),
 * element [b][u] of the [B][w] arrays:
 *   acc[0] += 1                      batches
 *   acc[1] += P                      positions
 *   acc[2] += S(nll)                 acc[3] += S(ptgt)
 *   acc[4] += S(arg-max class == target class, as 1.0 / 0.0), target[b][u] = (int)wav[b * wav_pitch + tgt_off + u + 1]
 *                                    (the target of aew_softmax_nll_t); the arg-max class is amax[b][u] or, with amax
 *                                    NULL, the LOWEST class c < n_quant holding the maximum of logits[b * bs + u * pitch + c]
 *                                    (a later class replaces an earlier one only where it is strictly greater: the rule
 *                                    of aew_softmax_nll_t.amax)
 *   acc[5] += Q                      acc[6] += S(dist[0:Q])      (ind != NULL only; dist may be NULL: nothing is added)
 *   acc[7] += loss[0]                acc[8 + j] += loss[1 + j], j < 4                       (loss != NULL only)
 *   hist[ind[q]] += 1 for q < Q      (integer atomics: exact in any order; an index outside [0, K) is not counted)
 *   acc[12..15] are not touched.
 * THE order of every floating sum S(x) over n elements: thread t (of 1024) adds the elements i = t, t + 1024, ...
 * ascending to a double that starts at 0.0, each element converted to double first; the 1024 partial sums go to LDS and
 * are folded by the halving tree  for (o = 512; o > 0; o >>= 1) s[t] += s[t + o] for t < o;  s[0] is the batch's sum,
 * and thread 0 adds it to acc with one double addition.  No floating atomics.
 *
 * finalize != 0: nothing is accumulated; out[0..15] are written from acc and hist (n / 0 = 0 throughout):
 *   out[0] acc[7] / acc[0]  mean loss per batch          out[1] acc[2] / acc[1]  nll per position (nats)
 *   out[2] out[1] / ln 2    bits per sample              out[3] acc[4] / acc[1]  top-1 accuracy
 *   out[4] acc[3] / acc[1]  mean target probability      out[5] acc[6] / acc[5]  mean dist
 *   out[6] entropy in bits of hist / sum(hist): -S(p_k log2 p_k) over the k with hist[k] > 0, in double, in THE order
 *   out[7] 2^out[6] (0 while sum(hist) == 0)              out[8] number of k with hist[k] > 0
 *   out[9 + j] acc[8 + j] / acc[0], j < 4  mean terms    out[13] acc[1]   out[14] acc[0]   out[15] 0
 * every quotient taken in double and rounded to fp32 once.  With hist == NULL out[6..8] are 0.
 *
 * Before any launch - accumulate: AEW_E_ARG for B < 1, w < 2 (no position left), a NULL acc / nll / ptgt / wav, neither
 * amax nor logits (or logits with n_quant < 1), ind with K < 1, Q < 1 or a NULL hist; finalize: AEW_E_ARG for a NULL
 * acc / out, hist with K < 1.  AEW_E_ALIGN (both): acc or ind not 8-byte aligned, any other pointer not 4-byte aligned. */
#define AEW_EVAL_ACC_N 16
#define AEW_EVAL_OUT_N 16
typedef struct {
    const float* nll; const float* ptgt;                    /* [B][w], as aew_softmax_nll_t wrote them                */
    const float* wav; int32_t wav_pitch; int32_t tgt_off;   /* the targets, as in aew_softmax_nll_t                   */
    int32_t B, w;
    const int32_t* amax;                                    /* [B][w] (aew_softmax_nll_t.amax), or NULL:              */
    const float* logits; int64_t bs; int32_t pitch; int32_t n_quant;   /* fp32 [B][w][>= n_quant]                     */
    const int64_t* ind; const float* dist; int32_t Q, K;    /* optional: code index / distance per query [Q]           */
    const float* loss;                                      /* optional [5]: aew_reduce_t.out of the evaluation's loss */
    double* acc;                                            /* [AEW_EVAL_ACC_N] the running record                     */
    uint32_t* hist;                                         /* [K] code counts (with ind; finalize: optional)          */
    int32_t finalize; int32_t pad_;
    float* out;                                             /* [AEW_EVAL_OUT_N], written by finalize only              */
} aew_eval_acc_t;

/* ---------------------------------------------------------------------------------------
 * Evaluation by group (appended to ABI 28; AEW_OP_EVAL_GROUPS, aew_sizeof 32): the sums of aew_eval_acc_t taken PER
 * WINDOW and folded into a record indexed by a per-window group id (the voice, or any labelling the caller has), and the
 * (group, code) contingency table from which the mutual information I(code; group) is read off - how much of the
 * grouping (speaker identity) the discrete codes carry.  It writes nothing a training step reads.
 *
 * finalize == 0 (accumulate).  nll, ptgt, wav / wav_pitch / tgt_off, B, w, amax or logits / bs / pitch / n_quant are those
 * of aew_eval_acc_t.  ind int64 [B * Qw] / dist [B * Qw] (optional): query q belongs to window q / Qw (b-major).  group
 * int64 [B].  nll == NULL selects CODES-ONLY mode: no position sums are taken (w, ptgt, wav, amax, logits are ignored),
 * only the queries are counted; ind is required.
 * The record (device memory, zeroed by the caller before the first batch):
 *   gacc  double [G][8]   per group: 0 windows, 1 positions (w - 1 per window; codes-only: none), 2 S(nll), 3 S(ptgt),
 *                         4 top-1 hits, 5 queries (Qw per window, with ind), 6 S(dist) (with ind and dist), 7 never written
 *   ghist uint32 [G][K]   the contingency table: ghist[group[b]][ind[q]] += 1 (integer atomics: exact in any order; a
 *                         query whose code lies outside [0, K) is not counted anywhere)
 *   gtot  double [4]      0: windows dropped because group[b] lies outside [0, G) - such a window is counted nowhere,
 *                         neither in its positions nor in its queries; 1: batches; 2, 3 never written
 *   win   double [B][4]   OVERWRITTEN by every accumulate launch: S(nll), S(ptgt), hits, S(dist) of window b alone (also
 *                         for a dropped window; codes-only: 0, 0, 0, S(dist))
 * Order of the floating sums (no floating atomics; two runs are bit-equal).  Per window: ONE workgroup of 1024 threads
 * owns window b; thread t adds the window's elements u = t, t + 1024, ... ascending, u < w - 1 (for dist: its queries
 * j < Qw ascending), each converted to double first, to a double that starts at 0.0; the 1024 partial sums are folded by
 * the halving tree  for (o = 512; o > 0; o >>= 1) s[t] += s[t + o] for t < o  - THE order and THE tree of aew_eval_acc_t -
 * and s[0] goes to win[b].  Per group: a second kernel, one thread per group, walks b = 0 .. B - 1 ascending and adds the
 * window sums of its group to gacc[g], one double addition per entry; counts are added as doubles (exact below 2^53).
 * So for B == 1, gacc[g][2..4] and [6] carry the bits aew_eval_acc_t adds to acc[2], acc[3], acc[4], acc[6].
 *
 * finalize != 0: nothing is accumulated; gout and tout are written from the record.  With n_gk = ghist[g][k],
 * n_g = sum_k n_gk, n_k = sum_g n_gk, N = sum n_gk (all integer); every quotient taken in double and rounded to fp32
 * once; x / 0 = 0; terms with n_gk == 0 are skipped:
 *   gout float [G][12]  per group: 0 windows, 1 positions, 2 nll per position gacc[2] / gacc[1], 3 bits per sample
 *                       ([2] / ln 2, in double), 4 top-1 gacc[4] / gacc[1], 5 mean target probability gacc[3] / gacc[1],
 *                       6 mean dist gacc[6] / gacc[5], 7 queries gacc[5], 8 E_g = -sum_k (n_gk / n_g) log2(n_gk / n_g),
 *                       9 2^E_g (0 if n_g == 0), 10 number of k with n_gk > 0, 11 0
 *   tout float [16]     0 N, 1 H(C) = -sum_k (n_k / N) log2(n_k / N), 2 H(G) = -sum_g (n_g / N) log2(n_g / N),
 *                       3 H(C|G) = sum_g (n_g / N) E_g, 4 I = (sum_g J_g) / N with
 *                       J_g = sum_k n_gk log2(((double)n_gk * N) / ((double)n_g * n_k)) - computed this way a table with
 *                       independent rows and columns gives 0 exactly -, 5 the Miller-Madow corrected value
 *                       I - (cells - rows - cols + 1) / (2 N ln 2) (cells, rows, cols: the numbers of non-zero n_gk, n_g,
 *                       n_k; NOT clamped, it may be slightly negative), 6 I / H(G), 7 I / H(C), 8 cells, 9 rows, 10 cols,
 *                       11 gtot[0] dropped windows, 12 gtot[1] batches, 13..15 0
 * Every sum over k (E_g, J_g, H(C)) follows THE order - thread t takes k = t, t + 1024, ... ascending - and THE tree; the
 * sums over g (H(G), H(C|G), sum J_g, cells) are taken ascending g by one thread, rows with n_g == 0 skipped.  With
 * ghist == NULL gout[.][8..10] are 0 and tout is zero except [11] and [12].
 * scratch (finalize with ghist only): 8-byte words [K + 4 * G], written by finalize - the column sums n_k as uint64 [K],
 * then per group n_g, E_g, J_g, cells_g as doubles.
 *
 * Before any launch - accumulate: AEW_E_ARG for B < 1, G < 1, a NULL group / gacc / gtot / win, ind with K < 1, Qw < 1
 * or a NULL ghist, codes-only without ind; unless codes-only: w < 2, a NULL ptgt / wav, neither amax nor logits (or
 * logits with n_quant < 1).  finalize: AEW_E_ARG for G < 1, a NULL gacc / gtot / gout / tout, ghist with K < 1 or a NULL
 * scratch.  AEW_E_ALIGN (both): gacc, gtot, win, ind, group or scratch not 8-byte aligned, any other pointer not 4-byte
 * aligned. */
#define AEW_EVAL_GACC_N 8
#define AEW_EVAL_GOUT_N 12
#define AEW_EVAL_TOUT_N 16
typedef struct {
    const float* nll; const float* ptgt;                    /* [B][w] (nll NULL: codes-only)                           */
    const float* wav; int32_t wav_pitch; int32_t tgt_off;
    int32_t B, w;
    const int32_t* amax;
    const float* logits; int64_t bs; int32_t pitch; int32_t n_quant;
    const int64_t* ind; const float* dist; int32_t Qw, K;   /* optional: [B * Qw], b-major                             */
    const int64_t* group; int32_t G; int32_t finalize;      /* [B] group id per window                                 */
    double* gacc; uint32_t* ghist; double* gtot; double* win;
    float* gout; float* tout;                               /* written by finalize only                                */
    void* scratch;                                          /* finalize with ghist: [K + 4 * G] 8-byte words           */
} aew_eval_groups_t;

/* ---------------------------------------------------------------------------------------
 * Per-parameter update / weight ratios (ABI 22): what the reference's training loop computes around optim.step()
 * (chassis.py:162-185: clone every parameter, step, norm(clone - p) / norm(clone) per tensor) - here from inside the
 * Adam launch, which holds the old and the new value of every element in registers: no clone, no extra pass over
 * memory, no host synchronisation, ONE summation order.
 *   chunk table : the host cuts the flat buffer into chunks (aew_uw_chunks): no chunk crosses a tensor boundary, a chunk
 *                 holds at most AEW_UW_CHUNK elements, tensors ascending, chunks ascending within a tensor, the pad
 *                 elements behind a tensor (each starts at a multiple of 4) belong to no chunk.
 *   Adam launch : aew_adam_t.track set - one block per chunk that overlaps the launch's element range
 *                 [base, base + n) of the flat buffer.  The per-element arithmetic is that of the untracked launch (the
 *                 same device function), so p / m / v come out bit for bit; the pad elements behind a chunk are updated
 *                 by its block, like the untracked launch updates them, and enter no sum.  Each block accumulates, in
 *                 fp64, sum (p_old - p_new)^2 - the difference taken in fp32, as the reference's `c - p` - and
 *                 sum p_old^2 over its part of the chunk: per thread one chain per sum (elements ascending), a fixed
 *                 butterfly inside the wave, waves ascending.  Thread 0 ADDS the pair to part[chunk] with plain loads
 *                 and stores: the launches of one step are ordered by the stream and no two blocks of a launch share
 *                 a chunk, so no atomics and the bits do not depend on the order of arrival.  `zero` != 0 (the first
 *                 launch of a step) clears part[] in front of the launch.
 *                 A step skipped on the device (guard word non-zero, clip[1] != 0) still reads p: it adds p_old^2 and
 *                 a zero difference - the step then reports an update norm of 0 and the true weight norm.
 *   reduce      : AEW_OP_UPDATE_RATIO (aew_update_ratio_t), one block per tensor.
 * ------------------------------------------------------------------------------------- */
#ifndef AEW_UW_CHUNK
#define AEW_UW_CHUNK 4096        /* elements per chunk = per block of the tracked Adam launch; a multiple of 1024          */
#endif
typedef struct {
    int64_t off;                 /* first element in the flat buffer (a multiple of 4)                                     */
    int32_t len;                 /* 1 .. AEW_UW_CHUNK                                                                      */
    int32_t tensor;              /* index of the tensor it belongs to                                                      */
} aew_uw_chunk_t;
/* The chunk table of tensors at flat offsets off[t] (multiples of 4, ascending, off[t + 1] >= off[t] + len[t]) with
 * len[t] >= 0 elements.  Writes the number of chunks to *n_chunks, the records to chunks[0 .. cap) when chunks != NULL
 * (AEW_E_ARG if cap is too small) and the first chunk of each tensor to first[0 .. n_tensors] when first != NULL
 * (first[n_tensors] = the number of chunks; a tensor of length 0 has none).  Host logic only: the engine, the tests and
 * the launcher's range arithmetic all read this one table. */
int aew_uw_chunks(const int64_t* off, const int64_t* len, int32_t n_tensors, aew_uw_chunk_t* chunks, int64_t cap,
                  int64_t* n_chunks, int32_t* first);
typedef struct {                 /* HOST record aew_adam_t.track points at (read at launch time only)                      */
    const aew_uw_chunk_t* chunks;        /* device copy of the table                                                      */
    const aew_uw_chunk_t* chunks_host;   /* host copy: the launcher finds the chunks that overlap [base, base + n) in it    */
    int64_t n_chunks;
    double* part;                /* device [n_chunks][2]: {sum (p_old - p_new)^2, sum p_old^2} per chunk, 16-byte aligned   */
    int64_t base;                /* flat offset of aew_adam_t.p[0] (a multiple of 4): the table speaks flat offsets          */
    int32_t zero;                /* != 0: clear part[] first (the first launch of a step)                                   */
    int32_t pad_;
} aew_uw_track_t;

/* ---------------------------------------------------------------------------------------
 * Parameter groups (appended to ABI 28; AEW_OP_ADAM_GROUPS, aew_adam_grouped_t below; aew_sizeof 29 / 30 / 31): per-tensor learning rate, decoupled weight decay and frozen
 * tensors inside the Adam launch - what torch.optim.AdamW with param groups and requires_grad_(False) do on the host.
 * Tensor t of the chunk table (aew_uw_chunk_t.tensor) carries a record (lr_t, decay_t, frozen_t).  The host computes
 * decay_t = 1 - lr_t * weight_decay_t in double and rounds it to fp32 ONCE.  For every element of tensor t, the pad
 * elements behind it up to the next multiple of 4 included:
 *   frozen_t != 0 : p, m, v and avg are not written; g, m, v and avg are not read.  With aew_adam_t.track the launch reads
 *                   p: the chunk adds p^2 to its weight sum and 0 to its update sum (update norm 0, the true weight norm,
 *                   ratio 0).  Without it a frozen chunk issues no memory access at all.
 *   else          : p1 = (decay_t == 1.0f) ? p : __fmul_rn(p, decay_t)         - decoupled decay FIRST (one rounding)
 *                   then the element update of every Adam launch on (p1, g, m, v) with step = lr_t / bc1 in place of
 *                   lr / bc1: torch.optim.AdamW.  bc1 / bc2 are those of the optimizer's ONE step count.
 *                   DEVIATION from torch, which keeps a step per parameter and no state for a frozen one: a tensor that
 *                   is unfrozen later continues with the global step and the moments it had when it was frozen.
 *   tracking      : the tracked p_old is the value in front of the decay (the update norm includes the decay's part).
 *   average       : avg moves towards p_new as in every launch; a frozen tensor's average keeps its bits.
 *   skipped steps : guard non-zero / clip[1] != 0 leave everything alone, as in every launch.
 * Clipping: the norm behind clip[0] is the caller's - it runs aew_grad_norm_t over the element ranges of the non-frozen
 * tensors only (torch.nn.utils.clip_grad_norm_ over the trainable parameters), in chained launches (finalize = 0 /
 * add_in) where there are more than AEW_GRAD_NORM_MAX_RANGES ranges.
 * Launch: one block per chunk that overlaps [base, base + n), the shape of the tracked launch; the block reads its tensor's
 * record once (uniform: scalar registers).  A range may begin or end inside a chunk at a multiple of 4; the n % 4 elements
 * at the very end of the buffer follow the tracked launch's rule.  aew_adam_t.lr is not read.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    float lr;                    /* lr_t                                                                                   */
    float decay;                 /* (float)(1.0 - (double)lr_t * (double)weight_decay_t); 1.0f = no decay, no multiply      */
    int32_t frozen;              /* != 0: the tensor is left alone                                                          */
    int32_t pad_;
} aew_adam_tensor_t;
typedef struct {                 /* HOST record aew_adam_grouped_t.groups points at (read at launch time only)             */
    const aew_uw_chunk_t* chunks;        /* device copy of the chunk table (aew_uw_chunks)                                 */
    const aew_uw_chunk_t* chunks_host;   /* host copy: the launcher finds the chunks that overlap [base, base + n) in it    */
    int64_t n_chunks;
    const aew_adam_tensor_t* tensors;    /* device [n_tensors], 16-byte aligned; read when the kernel runs                  */
    int32_t n_tensors;           /* every chunk's `tensor` the launch covers must lie in [0, n_tensors): AEW_E_ARG           */
    int32_t pad_;
    int64_t base;                /* flat offset of aew_adam_t.p[0] (a multiple of 4)                                        */
} aew_adam_groups_t;

typedef struct {                 /* fused Adam over a flat fp32 buffer (torch.optim.Adam defaults,
                                    checkpoint.py:49-50)                                      */
    float* p; const float* g; float* m; float* v;
    int64_t n;
    float lr, beta1, beta2, eps;
    float bc1, bc2;              /* 1-beta1^t, 1-beta2^t                                      */
    float grad_scale;            /* g is multiplied by this first (e.g. 1/world for a mean)   */
    int32_t pad_;
    const uint32_t* guard;       /* ABI 20, optional: device word read at launch time; non-zero = the update is a no-op.
                                    The engine points it at the STICKY word of its chained launches (aew_nt_chain_t.sticky):
                                    a step in which a hand-off wait gave up does not reach the parameters.              */
    const float* clip;           /* ABI 21, optional: device [2] = out[1..2] of an aew_grad_norm_t op of this step, read at launch
                                    time.  clip[1] != 0 (the gradient norm was inf / nan): the update is a no-op, like `guard`;
                                    else the gradient is g * grad_scale * clip[0], so the moments see the CLIPPED gradient
                                    (torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam).  clip[0] = 1.0f leaves every
                                    bit as without it.  A skipped step still counts on the HOST (bc1 / bc2 advance: the
                                    convention of `guard`).  NULL = no clipping: the kernel of ABI 20, bit for bit.          */
    const aew_uw_track_t* track; /* ABI 22, optional HOST pointer: also accumulate the update / weight sums of this launch's
                                    range per chunk (see above).  The chunks must cover [base, base + n): AEW_E_ARG otherwise,
                                    and for a NULL table / part or base < 0; AEW_E_ALIGN for base % 4 or part % 16.
                                    NULL = the launch of ABI 21, grid and bits.                                            */
    float* avg;                  /* ABI 24, optional: device buffer with the offsets of p (16-byte aligned: AEW_E_ALIGN) that holds
                                    an exponential moving average of the parameters.  The thread that updates an element also
                                    updates its average from the new parameter it still holds in a register:
                                        s = __fadd_rn(s, __fmul_rn(avg_rate, __fsub_rn(p_new, s)))
                                    - three round-to-nearest fp32 operations that the compiler may not contract into an FMA, so
                                    a numpy fp32 restatement gives the same bits.  Vector and scalar-tail paths alike, untracked
                                    and tracked launch alike; the pad elements behind a tensor are averaged like they are updated,
                                    and the tracked launch's sums (part[]) do not depend on it.  The per-element Adam arithmetic
                                    is untouched: p / m / v come out bit for bit as with avg = NULL.  A step the device skips
                                    (guard non-zero, clip[1] != 0) leaves avg untouched, like p / m / v.
                                    NULL = the launch of ABI 23, grid and bits.                                            */
    float avg_rate;              /* 1 - decay of this step, rounded to fp32 once by the host; with avg set it must lie in [0, 1]
                                    (AEW_E_ARG).  0 leaves avg as it is; 1 gives p_new up to the rounding of p_new - s.        */
    int32_t pad2_;
} aew_adam_t;

/* Exchange two flat fp32 buffers in place (ABI 24): a[i] <-> b[i] for i in [0, n).  One pass, float4 loads and stores with a
 * scalar tail; every element is read once and written once per buffer, no third buffer.  The engine swaps the parameters with
 * their average (aew_adam_t.avg) around sampling / evaluation.  n = 0 is a no-op.
 * AEW_E_ARG: n < 0, a NULL pointer with n > 0, buffers that overlap; AEW_E_ALIGN: a or b not 16-byte aligned. */
typedef struct { float* a; float* b; int64_t n; } aew_swap_t;

/* The Adam launch with parameter groups (appended to ABI 28; AEW_OP_ADAM_GROUPS, aew_sizeof 31): `adam` is the descriptor
 * of AEW_OP_ADAM, every field with its meaning there (clip, track, avg included; `lr` is not read), `groups` the HOST
 * record of aew_adam_groups_t above: per-tensor lr / decay / frozen, one block per chunk like a launch with `track`.
 * aew_adam_t itself is unchanged, so a plan built from AEW_OP_ADAM ops is byte for byte what it was.
 * Refused before any launch under the conditions of `track`: AEW_E_ARG for a NULL `groups`, chunks that do not cover
 * [base, base + n), a NULL table / tensors, base < 0, a chunk whose tensor lies outside the table, and - with adam.track
 * also set - a track record that names another table or base; AEW_E_ALIGN for base % 4 or tensors % 16, and whatever
 * AEW_OP_ADAM refuses.  A refused call writes nothing. */
typedef struct {
    aew_adam_t adam;
    const aew_adam_groups_t* groups;
} aew_adam_grouped_t;

/* Gradient accumulation (appended to ABI 28; aew_sizeof 25 - index 24 stays unused, it answers -1): fold the buffer a backward just wrote into a running sum, k micro-batches per optimizer
 * step.  One pass, float4 loads and stores with a scalar tail, a grid that depends on n only; plain vector loads and stores,
 * no atomics.  Every element gets ONE round-to-nearest fp32 addition that is never contracted with anything: a numpy fp32
 * `acc + g` gives the same bits, and the sum of a group is ((g1 + g2) + g3) + ... + gk whatever the launch geometry.
 * n = 0 is a no-op.  AEW_E_ARG: n < 0, a NULL pointer with n > 0, a mode outside 0..2, buffers that overlap;
 * AEW_E_ALIGN: acc or g not 16-byte aligned.  A refused call writes nothing. */
enum { AEW_ACCUM_FIRST = 0, AEW_ACCUM_ADD = 1, AEW_ACCUM_LAST = 2 };
typedef struct {
    float* acc;                  /* running sum [n], 16-byte aligned */
    float* g;                    /* the buffer a backward just wrote [n], 16-byte aligned */
    int64_t n;
    int32_t mode;                /* 0 FIRST: acc[i] = g[i]
                                    1 ADD  : acc[i] = __fadd_rn(acc[i], g[i])
                                    2 LAST : g[i]   = __fadd_rn(acc[i], g[i])   (acc is not written) */
    int32_t pad_;
} aew_accum_t;

/* Code sequences as data (appended to ABI 28; aew_sizeof 27 / 28 - index 26 stays unused, it answers -1).
 *
 * AEW_OP_CODE_LOOKUP: the inverse of AEW_OP_VQ_NEAREST on its zq output, same layouts -
 *     zq[q][j] = emb[ind[q]][j] for j < d,   zq[q][j] = 0 for d <= j < d_pitch,   q < Q.
 * It moves bytes only: the result equals numpy's emb[ind] bit for bit.  An index outside [0, K) is never followed - the
 * test comes before any load from emb: that row of zq is written as zeros and, with bad != NULL, the thread that owns the
 * row adds 1 to *bad (integer atomicAdd; the caller zeroes the word).  16-byte loads and stores where d, d_pitch are
 * multiples of 4 and emb, zq are 16-byte aligned, 4-byte ones otherwise.
 * AEW_E_ARG: Q, K or d < 1, d_pitch < d, a NULL ind / emb / zq; AEW_E_ALIGN: ind not 8-byte aligned, emb / zq / bad not
 * 4-byte aligned.  Both before any launch. */
typedef struct {
    const int64_t* ind;          /* [Q]                                                        */
    const float* emb;            /* [K][d]                                                     */
    float* zq;                   /* [Q][d_pitch]                                               */
    uint32_t* bad;               /* optional: += number of q with ind[q] outside [0, K)        */
    int32_t Q, K, d, d_pitch;
} aew_code_lookup_t;

/* AEW_OP_CODE_RUNS: run-length collapse of code rows (frames -> units).  Position t of row b starts a run iff t == 0 or
 * ind[b][t] != ind[b][t - 1].  With n = the number of runs of the row:
 *     units[b][r]   = the code of run r for r < n, -1 for n <= r < N
 *     lengths[b][r] = the length of run r for r < n, 0 for n <= r < N          n_runs[b] = n
 * One workgroup of 256 threads per row walks it in chunks of 1024 positions (four per thread) and carries the run count and
 * the position of the last start from chunk to chunk; inside a chunk a start's rank comes from its wave's ballot (popcount
 * of the lanes below) and the waves' counts meet in LDS.  Integer work only, no atomics, every output element is written exactly once:
 * the result is a pure function of the input.  Output sizes are fixed, so the op can sit in a captured graph.
 * AEW_E_ARG: B or N < 1, ind_pitch < N, a NULL pointer; AEW_E_ALIGN: ind / units not 8-byte aligned, lengths / n_runs not
 * 4-byte aligned.  Both before any launch. */
typedef struct {
    const int64_t* ind;          /* [B][ind_pitch], N codes per row                            */
    int64_t ind_pitch;           /* elements between rows (>= N)                               */
    int64_t* units;              /* [B][N]                                                     */
    int32_t* lengths;            /* [B][N]                                                     */
    int32_t* n_runs;             /* [B]                                                        */
    int32_t B, N;
} aew_code_runs_t;

/* Whole utterances through the fixed-geometry encoder (appended to ABI 28; AEW_OP_MEL_TILE / AEW_OP_CODE_STITCH,
 * aew_sizeof 34 / 35 / 36 - index 33 stays unused, it answers -1).  The encoder is a chain of valid convolutions of
 * stride s and receptive field rf mel frames, mel_len = s * (E - 1) + rf for E = embed_len codes per window.  An utterance of F frames has N = 0 codes if F < rf, else
 * (F - rf) / s + 1; its window w starts at frame w * s * E and holds the codes [w E, min(N, w E + E)).  The frames a window
 * lacks are zeros, and a code is stored only if its receptive field lies inside the real frames - so the codes of the
 * windows, put side by side, are those of one run over the whole utterance, bit for bit (the exact fp32 chain sums every
 * output frame in an order that depends on the K axis and not on the position).
 *
 * Both ops read one table of records in DEVICE memory, one record per batch row: the launch is given the table and the
 * first row of its batch, so a caller uploads the table of a whole call once and no launch waits for the host.  The
 * launchers check the rows [first_row, first_row + B) on `table_host`, a host copy of the same records (the pinned buffer
 * the upload was made from); the kernels repeat the check on the device copy and treat a record that fails it as idle
 * (zeros / nothing stored), so a captured graph whose table is rewritten between replays stays inside its buffers.
 * Plain loads and stores, no atomics, every loop bounded by the record.
 *
 * The ragged mel buffer holds the utterances' (n_mel, F_u) arrays one behind the other: channel c, frame t of a window
 * is element src + c * pitch + t. */
typedef struct {
    int64_t src;                 /* element offset of the window's first frame (channel 0) in the ragged mel buffer */
    int64_t dst;                 /* element offset of the window's first code in the ragged outputs                 */
    int32_t pitch;               /* elements between channels: the utterance's frame count                         */
    int32_t avail;               /* frames that exist from src on, 0 .. mel_len; 0: an idle row (src, pitch unused) */
    int32_t n_valid;             /* codes of the row that are stored, 0 .. E; 0: nothing (dst unused)               */
    int32_t pad_;
} aew_utt_row_t;

/* AEW_OP_MEL_TILE: for b < B, with r = table[first_row + b], in_mel[b][c][t] = mel[r.src + c * r.pitch + t] for
 * t < r.avail and +0.0f for r.avail <= t < mel_len; every element of in_mel[0 .. B) is written exactly once, nothing
 * else is.  16-byte stores where in_mel is 16-byte aligned and n_mel * mel_len a multiple of 4 (4-byte ones otherwise);
 * a window's first frame is only 4-byte aligned, so the loads are 16, 8 or 4 bytes wide as each address allows.
 * AEW_E_ARG: a NULL table / table_host / mel / in_mel, B < 1 or > 65535, first_row < 0, n_mel or mel_len < 1, n_src < 0,
 * a row with avail outside [0, mel_len] or - avail > 0 - src < 0, pitch < avail or a last element
 * src + (n_mel - 1) * pitch + avail - 1 outside [0, n_src); AEW_E_ALIGN: the tables not 8-byte, mel / in_mel not 4-byte
 * aligned.  All before any launch: a refused call writes nothing. */
typedef struct {
    const aew_utt_row_t* table;       /* device memory                                         */
    const aew_utt_row_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t first_row, B;
    const float* mel;            /* the ragged mel buffer, n_src elements                      */
    int64_t n_src;
    float* in_mel;               /* [B][n_mel][mel_len]                                        */
    int32_t n_mel, mel_len;
} aew_mel_tile_t;

/* AEW_OP_CODE_STITCH: for b < B, with r = table[first_row + b], codes[r.dst + j] = ind[b][j] and - dist != NULL -
 * dist[r.dst + j] = min_dist[b][j] for j < r.n_valid; it writes nothing else.  One wave per row, 8-byte (codes) and 4-byte
 * (distances) accesses: the widest a destination offset of any element count allows.
 * AEW_E_ARG: a NULL table / table_host / ind / codes, dist without min_dist, B < 1 or > 65535, first_row < 0, E < 1,
 * n_dst < 0, a row with n_valid outside [0, E] or - n_valid > 0 - [dst, dst + n_valid) outside [0, n_dst); AEW_E_ALIGN:
 * the tables / ind / codes not 8-byte, min_dist / dist not 4-byte aligned.  All before any launch. */
typedef struct {
    const aew_utt_row_t* table;       /* device memory                                         */
    const aew_utt_row_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t first_row, B;
    const int64_t* ind;          /* [B][E]: AEW_OP_VQ_NEAREST's indices of the batch           */
    const float* min_dist;       /* [B][E]: its distances (needed with dist only)              */
    int64_t* codes;              /* ragged output, n_dst elements                              */
    float* dist;                 /* optional ragged output, n_dst elements                     */
    int64_t n_dst;
    int32_t E, pad_;
} aew_code_stitch_t;

/* The index arithmetic of the two ops for one record, as the kernels and the launchers compute it (one __host__ __device__
 * definition; host-only export for tests): *avail / *n_valid = the frames AEW_OP_MEL_TILE copies / the codes
 * AEW_OP_CODE_STITCH stores, *src = the element of the ragged mel buffer that in_mel[b]'s flat element i (row-major
 * (n_mel, mel_len)) is copied from, -1 where it becomes zero.  AEW_E_ARG: a NULL pointer, n_mel / mel_len / E < 1,
 * n_src / n_dst < 0, i outside [0, n_mel * mel_len), or a record either launcher refuses. */
int aew_utterance_locate(const aew_utt_row_t* row, int n_mel, int mel_len, int E, int64_t n_src, int64_t n_dst, int64_t i,
                         int64_t* src, int32_t* avail, int32_t* n_valid);

/* Whole utterances through the fixed-geometry conditioning chain (appended to ABI 28; AEW_OP_CODE_TILE /
 * AEW_OP_COND_STITCH, aew_sizeof 37 / 38 / 39).  The chain codes -> codebook rows -> identity gather -> LC conv (k = 3,
 * valid) -> transposed-conv upsamplers (padding f - s) is shift-invariant and valid: a shift of one code moves the last
 * upsampler's output by S = prod(strides) rows, and no output row reads outside its inputs.  For n codes that output has
 * L(n) rows ("conditioning positions"); an engine of E = embed_len codes keeps T = dec_in_len of its L(E) rows from row
 * trim0 on.  With p = ceil(trim0 / S) and the hop h = (T - (p S - trim0)) / S codes, window w of an utterance of N codes
 * holds the codes [w h - p, w h - p + E) - code 0 where the utterance has none - and owns the conditioning positions
 * [w h S, min((w + 1) h S, L(N))): its cond rows from p S - trim0 on.  Row for row these are the bits of one run over
 * the whole code sequence (a row's sums depend on the K axis of its GEMMs, not on its position).
 *
 * Both ops read one table of records in DEVICE memory, one per batch row, as the whole-utterance encode's ops do: the
 * launchers check the rows [first_row, first_row + B) on `table_host` (the pinned buffer the upload was made from), the
 * kernels repeat the check on the device copy and treat a record that fails it as idle, so a captured graph whose table
 * is rewritten between replays stays inside its buffers. */
typedef struct {
    int64_t code0;               /* index in the flat code buffer of the window's code 0 (in front of the buffer or behind it
                                    where lo / hi keep the reads inside): window code j is codes[code0 + j]             */
    int32_t utt;                 /* the utterance, < 0: an idle row (nothing else of the record is used)                */
    int32_t stream;              /* its stream: cond_utt[stream], bias_utt[stream]                                      */
    int32_t lo, hi;              /* the window's codes [lo, hi) exist, 0 <= lo <= hi <= E; the others are code 0        */
    int32_t src_row;             /* first owned row of the window's cond, [src_row, src_row + n_rows) inside [0, T)     */
    int32_t n_rows;              /* owned rows                                                                          */
    int32_t dst_row;             /* conditioning position of the first owned row: its row in the stream's buffer        */
    int32_t pitch;               /* rows per stream of cond_utt; [dst_row, dst_row + n_rows) lies inside [0, pitch)     */
    int32_t voice;               /* the utterance's voice, [0, n_voice)                                                 */
    int32_t first;               /* != 0: the first window of its utterance (AEW_OP_COND_STITCH stores its bias)        */
} aew_cond_row_t;

/* AEW_OP_CODE_TILE: for b < B, with r = table[first_row + b]: ind[b][j] = codes[r.code0 + j] for r.lo <= j < r.hi, 0 for
 * the other j < E; in_voice[b] = r.voice; an idle row gets code 0 and voice 0.  A code outside [0, K) is written as 0 -
 * the lookup behind it never follows it - and counted in *bad (uint32, atomicAdd; windows overlap, so one bad code may
 * count more than once: test the word for non-zero).  One wave per row, 8-byte accesses.
 * AEW_E_ARG: a NULL table / table_host / codes / ind / in_voice / bad, B < 1 or > 65535, first_row < 0, E, K or n_voice
 * < 1, n_codes < 0, a live row with lo / hi outside 0 <= lo <= hi <= E, a read [code0 + lo, code0 + hi) outside
 * [0, n_codes) or a voice outside [0, n_voice); AEW_E_ALIGN: a pointer that is not 16-byte aligned (bad: 4-byte).  All
 * before any launch: a refused call writes nothing. */
typedef struct {
    const aew_cond_row_t* table;       /* device memory                                         */
    const aew_cond_row_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t first_row, B;
    const int64_t* codes;        /* the flat code buffer, n_codes elements                     */
    int64_t n_codes;
    int64_t* ind;                /* [B][E]: what AEW_OP_CODE_LOOKUP reads                      */
    int64_t* in_voice;           /* [B]                                                        */
    uint32_t* bad;               /* one device word, added to                                  */
    int32_t E, K;
    int32_t n_voice, pad_;
} aew_code_tile_t;

/* AEW_OP_COND_STITCH: for b < B, with r = table[first_row + b], the rows [r.src_row, r.src_row + r.n_rows) of cond[b]
 * (bf16, Cp channels, cond_pitch elements between rows, cond_bs between batch rows) go to the rows
 * r.stream * r.pitch + r.dst_row ... of cond_utt ([streams][r.pitch][Cp], contiguous); where r.first, bias[b][0:bias_n)
 * (fp32) goes to bias_utt[r.stream].  Nothing else is written: not an idle row's, not the rows of a stream behind its
 * last window (the caller zero-fills cond_utt once).  One launch for the B windows, 16-byte loads and stores.
 * AEW_E_ARG: a NULL table / table_host / cond / cond_utt / bias / bias_utt, B < 1 or > 65535, first_row < 0, T < 1,
 * Cp < 8 or no multiple of 8, cond_pitch < Cp or cond_pitch / cond_bs no multiple of 8, bias_n < 4 or no multiple of 4,
 * n_streams < 1, n_dst < 0, a live row with a source range outside [0, T), stream outside [0, n_streams), pitch < 1,
 * a destination range outside [0, pitch) or a stream buffer that ends behind n_dst elements; AEW_E_ALIGN: a pointer that is
 * not 16-byte aligned.  All before any launch. */
typedef struct {
    const aew_cond_row_t* table;
    const aew_cond_row_t* table_host;
    int32_t first_row, B;
    const uint16_t* cond;        /* dec.cond: [B] rows of T x Cp bf16                          */
    int64_t cond_bs;             /* elements between its batch rows                            */
    int32_t cond_pitch, T;       /* elements between its rows; rows per window                 */
    uint16_t* cond_utt;          /* n_dst elements                                             */
    int64_t n_dst;
    const float* bias;           /* [B][bias_n]: the gated bias of the batch (spk_bias)        */
    float* bias_utt;             /* [n_streams][bias_n]                                        */
    int32_t Cp, bias_n;
    int32_t n_streams, pad_;
} aew_cond_stitch_t;

/* Whole utterances through the teacher-forced decoder: the likelihood of a waveform given codes and a voice (appended to
 * ABI 28; AEW_OP_WAV_TILE / AEW_OP_NLL_STITCH / AEW_OP_SCORE_REDUCE, aew_sizeof 42 .. 45).  With rf = the sum of the
 * dilations and T = dec_in_len = w + rf, output position u of a window reads decoder-input rows [u, u + rf] and cond rows
 * [u, u + rf]; its target is decoder-input sample u + rf + 1, and u = w - 1 carries no loss.  In the coordinates of the
 * whole-utterance conditioning (position q of an utterance of N codes is waveform sample o + q, 0 <= q < L(N)) the scored
 * samples are q_t in [rf + 1, n_u), n_u = min(L(N), len(wav) - o).  With r0 = p S - trim0 and the hop
 * h_s = (w - 1 - r0) / S codes, window j holds the codes [j h_s - p, j h_s - p + E), its cond row 0 is position
 * a_j = j h_s S - r0, and it OWNS the outputs u in [r0, r0 + h_s S) whose target a_j + u + rf + 1 lies below n_u: every
 * row an owned output reads is a real row of the utterance.
 *
 * AEW_OP_WAV_TILE and AEW_OP_NLL_STITCH read one table of records in DEVICE memory, one per batch row, under the rules of
 * the conditioning ops above: the launchers check the rows [first_row, first_row + B) on `table_host`, the kernels repeat
 * the check on the device copy and treat a record that fails it as idle. */
typedef struct {
    int64_t code0;               /* index in the flat code buffer of the window's code 0: window code j is codes[code0 + j]  */
    int64_t wav_base;            /* element of the flat waveform buffer that holds the utterance's sample 0                 */
    int64_t wav_len;             /* samples of the utterance; [wav_base, wav_base + wav_len) lies inside [0, n_wav)         */
    int64_t wav0;                /* the utterance's sample that is the window's decoder-input row 0 (o + a_j; it may lie in
                                    front of the utterance, and wav0 + T behind it: those rows get the zero code)            */
    int64_t dst;                 /* element of the flat outputs the first owned output goes to                              */
    int32_t utt;                 /* the utterance, < 0: an idle row (nothing else of the record is used)                    */
    int32_t lo, hi;              /* the window's codes [lo, hi) exist, 0 <= lo <= hi <= E; the others are code 0            */
    int32_t voice;               /* the row's voice, [0, n_voice)                                                           */
    int32_t src;                 /* first owned output position u; [src, src + n_out) lies inside [0, w - 1)                */
    int32_t n_out;               /* owned outputs                                                                           */
} aew_score_row_t;

/* AEW_OP_WAV_TILE: for b < B, with r = table[first_row + b]: wav[b][wav_off + t] = wavs[r.wav_base + r.wav0 + t] for the
 * t < T with 0 <= r.wav0 + t < r.wav_len, `zero` (the zero-amplitude code) for the others and for an idle row; ind[b] and
 * in_voice[b] as AEW_OP_CODE_TILE writes them.  A sample outside [0, n_quant) (a NaN included) is written as `zero` - the
 * base gather indexes a table with it - and counted in *bad_wav; a code outside [0, K) is written as 0 and counted in
 * *bad_codes (uint32, integer atomicAdd; windows overlap, so one value may count more than once).  Nothing else of `wav`
 * is written.
 * AEW_E_ARG: a NULL pointer, B < 1 or > 65535, first_row < 0, E, K, n_voice, n_quant or T < 1, wav_off < 0,
 * wav_off + T > wav_pitch, n_codes or n_wav < 0, `zero` outside [0, n_quant), a live row with lo / hi outside
 * 0 <= lo <= hi <= E, a code read outside [0, n_codes), a voice outside [0, n_voice), wav_len < 0 or
 * [wav_base, wav_base + wav_len) outside [0, n_wav), |wav0| >= 2^40; AEW_E_ALIGN: a pointer off 16 bytes (bad_*: 4).  All
 * before any launch: a refused call writes nothing. */
typedef struct {
    const aew_score_row_t* table;       /* device memory                                         */
    const aew_score_row_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t first_row, B;
    const int64_t* codes;        /* the flat code buffer, n_codes elements                     */
    int64_t n_codes;
    const float* wavs;           /* the flat ragged waveform buffer (float-encoded mu-law values), n_wav elements */
    int64_t n_wav;
    int64_t* ind;                /* [B][E]                                                     */
    int64_t* in_voice;           /* [B]                                                        */
    float* wav;                  /* the engine's waveform input, [B][wav_pitch]                */
    uint32_t* bad_codes;         /* one device word each, added to                             */
    uint32_t* bad_wav;
    int32_t wav_pitch, wav_off;  /* elements between batch rows; first decoder-input sample (trim_dec_in[0]) */
    int32_t T, n_quant;
    int32_t E, K;
    int32_t n_voice;
    float zero;                  /* the zero-amplitude code                                    */
} aew_wav_tile_t;

/* AEW_OP_NLL_STITCH: for b < B, with r = table[first_row + b] and i < r.n_out, u = r.src + i:
 *   dst_nll[r.dst + i] = nll[b * w + u];   dst_ptgt[r.dst + i] = ptgt[b * w + u] (where dst_ptgt is given);
 *   dst_hit[r.dst + i] = 1 if the arg-max class of position (b, u) equals its target (int)wav[b][tgt_off + u + 1], else 0
 *   (where dst_hit is given).  The arg-max is amax[b * w + u] where the softmax op wrote one, else the scan of
 *   logits[b * bs + u * pitch + 0 .. n_quant) in which the lowest class keeps a tie - the rule of aew_eval_acc_t.
 * Nothing outside the owned ranges is written.
 * AEW_E_ARG: a NULL table / table_host / nll / dst_nll, dst_ptgt without ptgt, dst_hit without wav or without both amax
 * and logits (n_quant >= 1, pitch >= n_quant, bs >= 0), B < 1 or > 65535, first_row < 0, w < 2, tgt_off < 0,
 * tgt_off + w > wav_pitch, n_dst < 0, a live row with [src, src + n_out) outside [0, w - 1) or [dst, dst + n_out) outside
 * [0, n_dst); AEW_E_ALIGN: table / table_host off 16 bytes, a float / int32 pointer off 4.  All before any launch. */
typedef struct {
    const aew_score_row_t* table;
    const aew_score_row_t* table_host;
    int32_t first_row, B;
    const float* nll;            /* [B][w]: what AEW_OP_SOFTMAX_NLL wrote                      */
    const float* ptgt;           /* [B][w] (optional)                                          */
    const int32_t* amax;         /* [B][w] (optional)                                          */
    const float* logits;         /* (optional; read where amax is NULL)                        */
    int64_t bs;                  /* elements between the batch rows of logits                  */
    const float* wav;            /* the engine's waveform input, [B][wav_pitch]                */
    float* dst_nll;              /* n_dst elements                                             */
    float* dst_ptgt;             /* n_dst elements (optional)                                  */
    uint8_t* dst_hit;            /* n_dst elements (optional)                                  */
    int64_t n_dst;
    int32_t pitch, n_quant;      /* elements between the rows of logits; classes               */
    int32_t wav_pitch, tgt_off;
    int32_t w, pad_;
} aew_nll_stitch_t;

/* AEW_OP_SCORE_REDUCE: one workgroup of 1024 threads per utterance u < U over the stitched flat arrays, elements
 * [offsets[u], offsets[u + 1]) = n of them:
 *   acc[u] = (n, sum nll, sum ptgt, sum hit) as doubles - THE order and THE tree of aew_eval_acc_t: thread t adds its
 *            elements t, t + 1024, ... ascending into a double, then for (o = 512; o > 0; o >>= 1) s[t] += s[t + o] for
 *            t < o.  No floating atomics.  ptgt / hit may be NULL: their sums are 0.
 *   out[u] = (nll per sample, bits per sample = that / ln 2, top-1 = sum hit / n, mean target probability): quotients in
 *            double, rounded to fp32 once; all 0 where n = 0.
 * The sums run over the flat arrays, so they depend neither on the batch size nor on the tiling that filled them.
 * AEW_E_ARG: a NULL offsets / offsets_host / nll / acc / out, U < 1 or > 2^20, n_src < 0, offsets_host[0] < 0, a
 * decreasing pair or offsets_host[U] > n_src; AEW_E_ALIGN: offsets / acc off 8 bytes, nll / ptgt / out off 4.  The kernel
 * repeats the range check on the device copy and treats a failing utterance as empty. */
typedef struct {
    const int64_t* offsets;      /* device memory, [U + 1]                                     */
    const int64_t* offsets_host; /* the same numbers in host memory (read by the launcher)     */
    const float* nll;            /* n_src elements                                             */
    const float* ptgt;           /* (optional)                                                 */
    const uint8_t* hit;          /* (optional)                                                 */
    int64_t n_src;
    double* acc;                 /* [U][4]                                                     */
    float* out;                  /* [U][4]                                                     */
    int32_t U, pad_;
} aew_score_reduce_t;

/* Comparing utterances (appended to ABI 28; AEW_OP_SEQ_ALIGN, aew_sizeof 47 / 48 / 49): dynamic time warping over two
 * sequences of D-channel fp32 frames, or the Levenshtein distance of two strings of int64 symbols, for n_pairs
 * independent pairs in one launch.  One wavefront owns a pair from start to end; nothing in the op waits on another
 * wavefront - no flag, no spin, no barrier.
 *
 * THE RULE (tests/seq_align_emulator.py restates it).  fp32 throughout, every operation rounded on its own (no fused
 * multiply-add).  With n = len(a), m = len(b):
 *   local distance   acc = 0; for k = 0 .. D-1: t = a[i][k] - b[j][k]; acc = acc + t * t.
 *                    d(i, j) = acc (SQEUCLID) or the correctly rounded square root of acc (EUCLID).
 *   DTW              C(0,0) = d(0,0), S(0,0) = 1; otherwise C(i,j) = d(i,j) + C(pred), S(i,j) = S(pred) + 1 with pred the
 *                    EXISTING predecessor of least C among (i-1,j-1), (i-1,j), (i,j-1) - ties go to the first in that
 *                    order (strict < while scanning in that order).  cost = C(n-1,m-1), steps = S(n-1,m-1).
 *                    An empty side: cost = +inf, steps = 0, no feature memory is read.  A pair in which any d(i,j) is not
 *                    finite: cost = NaN, steps = 0, and *bad is raised by one (uint32, integer atomicAdd).
 *   EDIT             unit-cost Levenshtein distance of the symbols (compared as 64-bit integers, never used as an index;
 *                    D must be 1, chan_stride is not read).  An empty side: the other side's length.  steps = the distance,
 *                    cost = the same number as a float.
 *   path (DTW, when back and path are given)  back[back_base + i * m + j] = 0, 1 or 2: the predecessor of cell (i, j) in
 *                    the order above (0 for cell (0,0), which has none).  A second kernel of the SAME op launch, ordered
 *                    behind the first by the stream alone, walks back from (n-1, m-1) and writes the `steps` cells (i, j)
 *                    from start to end as int32 pairs at path[2 * (path_base + e)], e < steps; the entries
 *                    steps <= e < n + m - 1 are (-1, -1).  A pair with steps = 0 (not finite) has all n + m - 1 entries
 *                    (-1, -1) and its back bytes are unspecified; a pair with an empty side owns neither back nor path
 *                    elements.
 * Element (i, k) of a sequence is feat[base + i * frame_stride + k * chan_stride]: frame-major embeddings (frame_stride
 * = D, chan_stride = 1) and channel-major (channels, frames) arrays (frame_stride = 1, chan_stride = frames) are read in
 * place.
 * Every D in [1, AEW_ALIGN_MAX_D] gives these bits; D <= 64 holds the A row of a lane in registers.
 *
 * Tables: the A-side and B-side sequence tables and the pair table each come as a device copy and a host copy with the
 * same records (the convention of aew_wav_tile_t).  The launcher checks every record of the host copies against the
 * buffer sizes before anything is launched; the kernels repeat the checks on the device copies and leave a pair whose
 * records fail them alone (nothing of it is written): no address is formed from an unchecked record.
 * AEW_E_ARG: mode / metric outside their values, D outside [1, AEW_ALIGN_MAX_D] (EDIT: D != 1), n_pairs < 1 or > 2^24,
 * n_a / n_b < 1, a NULL table, cost, steps or bad, a NULL feature buffer of n_feat > 0, n_feat outside [0, 2^50], a
 * sequence with len outside [0, AEW_ALIGN_MAX_LEN], a negative stride or one above 2^40, base outside [0, n_feat) or an
 * element (len-1, D-1) at or behind n_feat; a pair with a / b outside its table; `path` without `back` or either in EDIT
 * mode; with back: back_base < 0 or back_base + n * m > n_back, path (where given) path_base < 0 or path_base + n + m - 1
 * > n_path; a pair of more than 64 A frames without a workspace of the size stated at `ws`.  AEW_E_ALIGN: a table off 8
 * bytes, int64 symbols off 8, any other pointer off 4.  A refused call launches and writes nothing. */
#define AEW_ALIGN_DTW 0
#define AEW_ALIGN_EDIT 1
#define AEW_ALIGN_EUCLID 0
#define AEW_ALIGN_SQEUCLID 1
#define AEW_ALIGN_MAX_D 256
#define AEW_ALIGN_MAX_LEN (1 << 20)
typedef struct {
    int64_t base;                /* element of the side's buffer that holds (frame 0, channel 0)                */
    int64_t frame_stride;        /* elements between frames                                                     */
    int64_t chan_stride;         /* elements between channels                                                   */
    int32_t len;                 /* frames (symbols); 0 is allowed                                              */
    int32_t pad_;
} aew_align_seq_t;

typedef struct {
    int32_t a, b;                /* indices into the A-side / B-side sequence tables                            */
    int64_t back_base;           /* first byte of the pair's n * m back-pointers in `back`                      */
    int64_t path_base;           /* first (i, j) entry of the pair's n + m - 1 in `path` (int32 element 2 * path_base) */
} aew_align_pair_t;

typedef struct {
    int32_t mode, metric;        /* AEW_ALIGN_DTW / _EDIT; AEW_ALIGN_EUCLID / _SQEUCLID (DTW)  */
    int32_t D, n_pairs;
    const aew_align_seq_t* seq_a;       /* device memory, n_a records                         */
    const aew_align_seq_t* seq_a_host;  /* the same records in host memory                    */
    const aew_align_seq_t* seq_b;
    const aew_align_seq_t* seq_b_host;
    const aew_align_pair_t* pairs;      /* device memory, n_pairs records                     */
    const aew_align_pair_t* pairs_host;
    int32_t n_a, n_b;
    const void* feat_a;          /* fp32 (DTW) or int64 (EDIT), n_feat_a elements              */
    const void* feat_b;
    int64_t n_feat_a, n_feat_b;
    float* cost;                 /* [n_pairs]                                                  */
    int32_t* steps;              /* [n_pairs]                                                  */
    uint32_t* bad;               /* one device word, added to                                  */
    void* ws;                    /* boundary rows of pairs with more than 64 A frames (optional): ws_bytes >= 8 * n_pairs *
                                    the longest B side among those pairs (the launcher takes that length from the host
                                    tables).  Contents are scratch.                                                        */
    int64_t ws_bytes;
    uint8_t* back;               /* n_back bytes (optional, DTW)                               */
    int64_t n_back;
    int32_t* path;               /* n_path (i, j) entries = 2 * n_path int32 (optional, needs back) */
    int64_t n_path;
} aew_seq_align_t;

/* Segmenting utterances (appended to ABI 28; AEW_OP_FRAME_STITCH / AEW_OP_CODE_SEGMENT, aew_sizeof 51 / 52 / 53 -
 * index 50 stays unused, it answers -1): the
 * code sequence of a whole utterance chosen JOINTLY - the labelling that minimises
 *     sum over frames of the distance to the chosen entry  +  lam * (number of code changes)
 * by a Viterbi pass over the K codebook entries with a uniform switch cost, U independent utterances in one launch.  One
 * wavefront owns an utterance's pass from start to end; nothing in the op waits on another wavefront - no flag, no spin,
 * no barrier.
 *
 * THE RULE (tests/segment_emulator.py restates it).  Inputs of one utterance: T >= 1 fp32 frames z_t of d values at pitch
 * d_pitch, the codebook emb[K][d], the metric (0 scaled_l2, 1 sq_l2, the meanings of aew_vq_nearest_t) and lam >= 0 (+inf
 * allowed).  fp32 throughout, every operation rounded on its own.
 *   local cost       c(t,k) is the value AEW_OP_VQ_NEAREST compares for query z_t and entry k, the same operations in
 *                    the same order: dd = 0, qq = 0; for j ascending: u = z_t[j] - e_k[j]; dd = fma(u, u, dd);
 *                    qq = fma(e_k[j], e_k[j], qq).  sq_l2: c = dd.  scaled_l2: zz = 0; for j ascending:
 *                    zz = fma(z_t[j], z_t[j], zz); c = sqrt(dd) / (sqrt(zz) + sqrt(qq)), sqrt and the division correctly
 *                    rounded.
 *   recurrence       r(0,k) = c(0,k); acc = 0
 *                    for t = 1 .. T-1:
 *                        m = +inf; a = 0; for k ascending: if r(t-1,k) < m: m = r(t-1,k); a = k
 *                                                       (the lowest index among ties; a NaN never wins)
 *                        A(t-1) = a; acc = acc + m
 *                        p(k) = r(t-1,k) - m;  stay(t,k) = p(k) < lam  (false for a NaN)
 *                        r(t,k) = c(t,k) + (stay(t,k) ? p(k) : lam)
 *                    (m, a) of r(T-1, .) as above; cost = acc + m; k = a
 *   walk back        for t = T-1 .. 1: codes[t] = k; if not stay(t,k): k = A(t-1).   codes[0] = k
 *   outputs          dist[t] = c(t, codes[t]); n_seg = 1 + #{t >= 1 : codes[t] != codes[t-1]}
 * The minimum is taken out at every step: the values stay at the scale of one frame's distances however long the
 * utterance is, and lam = 0 gives r(t,k) = c(t,k) exactly - codes and dist are then those of AEW_OP_VQ_NEAREST bit for
 * bit, ties included.  lam = +inf gives one code for the whole utterance.  The rule is total: an utterance whose cost
 * is not finite (a NaN or inf frame) still gets the outputs above and raises *n_bad by one (uint32, integer atomicAdd).
 * T = 0: cost = 0, n_seg = 0, no code is written.
 *
 * Utterance u is the rows [first_frame, first_frame + n_frames) of the ragged frame buffer; its codes and distances go to
 * the same indices of the flat outputs.  With W = ceil(K / 64) it owns the 64-bit words [back_base, back_base +
 * n_frames * (W + 1)) of the workspace's back region: per frame t the W words of stay(t, .) (bit k & 63 of word k >> 6)
 * and one word holding A(t-1).
 *
 * Workspace: the bytes aew_segment_ws_bytes(n_rows, K) states, 8-byte aligned - the [n_rows][K] fp32 local costs of ALL rows of the
 * frame buffer (n_rows * K * 4 bytes, rounded up to 8), then the back region of n_rows * (W + 1) words.  Contents are
 * scratch.  n_rows = the rows that lie inside n_elems: 0 if n_elems < d, else (n_elems - d) / d_pitch + 1.
 *
 * The table comes as a device copy and a host copy with the same records.  The launcher checks every record of the host
 * copy before anything is launched; the kernels repeat the record checks on the device copy and leave an utterance whose
 * record fails them alone (nothing of it is written).
 * AEW_E_ARG: a NULL emb / table / table_host / codes / cost / n_seg / n_bad / ws, NULL frames with n_elems > 0, metric
 * outside {0, 1}, K outside [1, AEW_SEG_MAX_K], d < 1 or > AEW_SEG_MAX_D, d_pitch < d, U < 0 or > 2^24, n_elems < 0,
 * n_out < n_rows, ws_bytes below what aew_segment_ws_bytes states; a record with n_frames < 0, lam negative or NaN, or -
 * n_frames > 0 - rows outside [0, n_rows), a back range outside the back region, or a back range that overlaps that
 * of another record.  AEW_E_ALIGN: table / table_host / codes / ws off 8 bytes, any other pointer off 4.  A refused
 * call launches and writes nothing; U = 0 launches nothing. */
#define AEW_SEG_MAX_K 4096
#define AEW_SEG_MAX_D 4096
typedef struct {
    int64_t first_frame;         /* first row of the utterance in the ragged frame buffer (and in codes / dist)   */
    int64_t back_base;           /* first 64-bit word of its n_frames * (W + 1) in the workspace's back region    */
    int32_t n_frames;            /* T; 0 is allowed                                                               */
    float lam;                   /* the switch penalty, >= 0, +inf allowed                                        */
} aew_seg_utt_t;

typedef struct {
    const float* frames;         /* ragged [n_rows][d_pitch] fp32                              */
    int64_t n_elems;             /* elements of `frames`                                       */
    const float* emb;            /* [K][d]                                                     */
    int32_t K, d, d_pitch;
    int32_t metric;              /* 0 scaled_l2, 1 sq_l2                                       */
    const aew_seg_utt_t* table;       /* device memory, U records                              */
    const aew_seg_utt_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t U, pad_;
    int64_t* codes;              /* flat output, n_out elements                                */
    float* dist;                 /* optional flat output, n_out elements                       */
    int64_t n_out;
    float* cost;                 /* [U]                                                        */
    int32_t* n_seg;              /* [U]                                                        */
    uint32_t* n_bad;             /* one device word, added to                                  */
    void* ws;
    int64_t ws_bytes;
} aew_code_segment_t;

/* *bytes = the workspace an AEW_OP_CODE_SEGMENT over a frame buffer of n_rows rows needs; AEW_E_ARG for a NULL pointer,
 * n_rows outside [0, 2^40] or K outside [1, AEW_SEG_MAX_K].  Host-only. */
int aew_segment_ws_bytes(int64_t n_rows, int K, int64_t* bytes);

/* The host twin of AEW_OP_CODE_SEGMENT: the same descriptor with every pointer in HOST memory (table is not read,
 * table_host is), the launcher's checks and then the rule on the CPU through the one __host__ __device__ definition of
 * the local cost, the recurrence step and the walk back that the kernels run (fmaf in place of __fmaf_rn).  The CPU
 * tests run this very code. */
int aew_segment_host(const aew_code_segment_t* p);

/* AEW_OP_FRAME_STITCH does for the encoder outputs what AEW_OP_CODE_STITCH does for the indices: for b < B, with
 * r = table[first_row + b], frames[(r.dst + j) * d_pitch + c] = lin[b * lin_bs + j * d_pitch + c] for j < r.n_valid,
 * c < d_pitch; it writes nothing else.  The same aew_utt_row_t table and the same record check (n_valid in [0, E],
 * [dst, dst + n_valid) inside [0, n_dst) rows); a record that fails it on the device copy stores nothing.  16-byte
 * moves where d_pitch and lin_bs are multiples of 4 and both buffers 16-byte aligned, 4-byte ones otherwise.
 * AEW_E_ARG: a NULL table / table_host / lin / frames, B < 1 or > 65535, first_row < 0, E < 1, d_pitch < 1,
 * lin_bs < E * d_pitch, n_dst < 0 or a row the check refuses; AEW_E_ALIGN: the tables not 8-byte, lin / frames not
 * 4-byte aligned.  All before any launch. */
typedef struct {
    const aew_utt_row_t* table;       /* device memory                                         */
    const aew_utt_row_t* table_host;  /* the same records in host memory (read by the launcher) */
    int32_t first_row, B;
    const float* lin;            /* [B][E][d_pitch], batch stride lin_bs elements              */
    int64_t lin_bs;
    float* frames;               /* ragged output, n_dst rows of d_pitch                       */
    int64_t n_dst;
    int32_t E, d_pitch;
} aew_frame_stitch_t;

/* Finding a query inside utterances (appended to ABI 28; AEW_OP_SEQ_SEARCH, aew_sizeof 55 / 56 - index 54 stays unused,
 * it answers -1): subsequence dynamic time warping of a query a (n frames) against a document b (m frames) - the match
 * may start and end at any document frame - for n_pairs independent pairs in one op, then the n_hits best
 * non-overlapping matches of each pair.  Two launches of the one op, ordered by the stream alone: the sweep (one
 * wavefront per pair, the shape of AEW_OP_SEQ_ALIGN's DTW kernel) and the pick (one wavefront per pair).  Nothing waits
 * on another wavefront - no flag, no spin, no barrier, no atomic but the count of pairs that are not finite.
 *
 * THE RULE (tests/seq_search_emulator.py restates it).  The arithmetic is AEW_OP_SEQ_ALIGN's: fp32 throughout, every
 * operation rounded on its own, d(i, j) that op's local distance for the metrics EUCLID and SQEUCLID over D channels.
 *   sweep    Row 0 starts a match anywhere: C(0,j) = d(0,j), S(0,j) = 1, B(0,j) = j for every j (row 0 has no left
 *            predecessor).  For i >= 1, pred = the EXISTING predecessor of least C among (i-1,j-1), (i-1,j), (i,j-1), ties to
 *            the first in that order (strict < while scanning in that order, exactly as DTW does); then
 *            C(i,j) = d(i,j) + C(pred), S(i,j) = S(pred) + 1, B(i,j) = B(pred).
 *   profile  The pair's m entries from prof_base on: end_cost[j] = C(n-1,j), end_steps[j] = S(n-1,j), end_start[j] =
 *            B(n-1,j).  The match that ends at document frame j starts at frame end_start[j].
 *   pick     key[j] = end_cost[j] / (float)end_steps[j], the correctly rounded fp32 quotient (rank MEAN), or end_cost[j]
 *            (rank COST).  An end is eligible when its key is finite and min_len <= j - end_start[j] + 1 and, when
 *            max_len > 0, that length is <= max_len.  For r = 0 .. n_hits-1: take the eligible, unsuppressed end of least
 *            key, ties to the least j; write hit r = (start, end, cost, steps); then suppress every end k whose interval
 *            [end_start[k], k] meets [start, end], that is end_start[k] <= end and k >= start.  count[p] = the hits
 *            found; the remaining hit slots are (-1, -1, +inf, 0).
 *   special  An empty side reads no feature memory.  m = 0 owns no profile entries; n = 0, m > 0 writes (+inf, 0, -1) to
 *            each; in both cases count = 0 and all hits are empty.  A pair with any d(i,j) not finite gets every profile
 *            entry (NaN, 0, -1), count = 0, empty hits, and *bad is raised by one (DTW's convention).
 *   caveat   The symmetric step pattern lets a match collapse onto one document frame; min_len / max_len are the remedy
 *            on offer, the step pattern itself does not change.
 *   slices   For every end j, C(n-1,j) is, bit for bit, the closed DTW cost of a against b[B(n-1,j) .. j] under
 *            AEW_OP_SEQ_ALIGN (and S the steps wherever no tie decides the path).
 * Tables and checks follow AEW_OP_SEQ_ALIGN: the two aew_align_seq_t tables (reused unchanged) and the pair table each
 * come as a device copy and a host copy; the launcher checks every host record before anything is launched, the kernels
 * repeat the checks on the device copies and leave a failing pair alone; no address is formed from an unchecked record.
 * The profile ranges [prof_base, prof_base + m) of the pairs must be disjoint - the caller's contract (prefix sums).
 * AEW_E_ARG: metric / rank outside their values, D outside [1, AEW_ALIGN_MAX_D], n_pairs < 1 or > 2^24, n_a / n_b < 1,
 * n_hits outside [1, AEW_SEARCH_MAX_HITS], min_len or max_len negative, a NULL table or output (prof_*, hits, hit_cost,
 * hit_steps, count, bad), a NULL feature buffer of n_feat > 0, n_feat outside [0, 2^50], n_prof < 0, a sequence record
 * AEW_OP_SEQ_ALIGN refuses, a pair with a / b outside its table, prof_base < 0 or prof_base + m > n_prof, a query of more
 * than 64 frames without a workspace of the size stated at `ws`.  AEW_E_ALIGN: a table off 8 bytes, any other pointer
 * off 4.  A refused call launches and writes nothing. */
#define AEW_SEARCH_MEAN 0
#define AEW_SEARCH_COST 1
#define AEW_SEARCH_MAX_HITS 32
typedef struct {
    int32_t a, b;                /* indices into the query / document sequence tables                           */
    int64_t prof_base;           /* first of the pair's m entries in prof_cost / prof_steps / prof_start         */
} aew_search_pair_t;

typedef struct {
    int32_t metric, rank;        /* AEW_ALIGN_EUCLID / _SQEUCLID; AEW_SEARCH_MEAN / _COST       */
    int32_t D, n_pairs;
    int32_t n_hits, min_len, max_len, pad_;   /* max_len 0: no upper limit                      */
    const aew_align_seq_t* seq_a;       /* the queries: device memory, n_a records             */
    const aew_align_seq_t* seq_a_host;  /* the same records in host memory                     */
    const aew_align_seq_t* seq_b;       /* the documents                                       */
    const aew_align_seq_t* seq_b_host;
    const aew_search_pair_t* pairs;     /* device memory, n_pairs records                      */
    const aew_search_pair_t* pairs_host;
    int32_t n_a, n_b;
    const float* feat_a;         /* n_feat_a elements                                          */
    const float* feat_b;
    int64_t n_feat_a, n_feat_b;
    float* prof_cost;            /* [n_prof]                                                   */
    int32_t* prof_steps;         /* [n_prof]                                                   */
    int32_t* prof_start;         /* [n_prof]                                                   */
    int64_t n_prof;
    int32_t* hits;               /* [n_pairs][n_hits][2]: (start, end) document frames         */
    float* hit_cost;             /* [n_pairs][n_hits]                                          */
    int32_t* hit_steps;          /* [n_pairs][n_hits]                                          */
    int32_t* count;              /* [n_pairs]; between the two launches it carries the sweep's verdict on the pair */
    uint32_t* bad;               /* one device word, added to                                  */
    void* ws;                    /* boundary rows (C, S, B) of pairs with more than 64 query frames (optional): ws_bytes >=
                                    12 * n_pairs * the longest document among those pairs (the launcher takes that length
                                    from the host tables).  Contents are scratch.                                          */
    int64_t ws_bytes;
} aew_seq_search_t;

/* Discovering repeats between utterances (appended to ABI 28; AEW_OP_SEQ_DISCOVER, aew_sizeof 61 / 62 - index 60 stays
 * unused, it answers -1): local-alignment dynamic time warping (segmental DTW) of a (n frames) against b (m frames) -
 * the alignment may start and end at any cell, nobody names a query - for n_pairs independent pairs in one op, then the
 * n_hits best alignments of each pair whose A ranges do not overlap.  Two launches of the one op, ordered by the stream
 * alone: the sweep (one wavefront per pair, the shape of AEW_OP_SEQ_ALIGN's DTW kernel) and the pick (one wavefront per
 * pair).  Nothing waits on another wavefront - no flag, no spin, no barrier, no atomic but the count of pairs that are
 * not finite.
 *
 * THE RULE (tests/seq_discover_emulator.py restates it).  The arithmetic is AEW_OP_SEQ_ALIGN's: fp32 throughout, every
 * operation rounded on its own, d(i, j) that op's local distance for the metrics EUCLID and SQEUCLID over D channels.
 * `threshold` is one finite fp32 for the launch, `band` >= 0 one int32 per pair.
 *   gain     g(i, j) = threshold - d(i, j), one fp32 subtraction.
 *   dead     Cell (i, j) lies OUTSIDE THE BAND when band > 0 and j - i < band: it is dead, H = 0 and S = 0, whatever d is.
 *            A pair of one utterance with itself (band >= 1) so looks only at the upper triangle, away from the trivial
 *            diagonal.  band = 0: every cell is inside.
 *   sweep    For a cell inside the band, scan the predecessors (i-1,j-1), (i-1,j), (i,j-1) that exist and have H > 0 in
 *            that order and keep the one of largest H (strict > while scanning: ties go to the first).  With such a
 *            predecessor H(i,j) = H(pred) + g(i,j), S(i,j) = S(pred) + 1, O(i,j) = O(pred); without one H(i,j) = g(i,j),
 *            S(i,j) = 1, O(i,j) = (i, j).  If the resulting H is not > 0 the cell is dead: H = 0, S = 0.  H is the score
 *            of the best local alignment that ends at the cell, S its cells, O = (row, column) the cell it starts at.
 *   profile  The pair's n entries from prof_base on, one per ROW i: E(i) = max over j of H(i,j) and, of the LEAST such j,
 *            prof_end[i] = j, prof_row[i] / prof_col[i] = O(i,j), prof_steps[i] = S(i,j).  E(i) = 0 - no alignment ends in
 *            this row - gives (0, -1, -1, -1, 0).
 *   pick     Row i is eligible when E(i) > 0 and both spans, i - prof_row[i] + 1 and prof_end[i] - prof_col[i] + 1, are
 *            >= min_len and, when max_len > 0, <= max_len.  For r = 0 .. n_hits-1: take the eligible, unsuppressed row
 *            of largest E, ties to the least i; write hit r = (a_start, a_end, b_start, b_end) = (prof_row[i], i,
 *            prof_col[i], prof_end[i]) with score E(i) and steps prof_steps[i]; then suppress every row k whose own A
 *            range [prof_row[k], k] meets [a_start, a_end], that is prof_row[k] <= a_end and k >= a_start.  count[p] =
 *            the hits found; the remaining hit slots are (-1, -1, -1, -1), NaN, 0.
 *   special  An empty side reads no feature memory: count = 0, all hits empty; n > 0, m = 0 writes (0, -1, -1, -1, 0) to
 *            each of the n profile entries, n = 0 owns none.  A pair in which d(i,j) is not finite for any cell INSIDE
 *            the band gets every profile entry (NaN, -1, -1, -1, 0), count = 0, empty hits, and *bad is raised by one
 *            (DTW's convention); what lies outside the band is not looked at.
 *   mean     steps * threshold - score is the summed local distance along a hit up to rounding, so threshold - score /
 *            steps its mean distance per cell; the closed DTW of the hit's two ranges under AEW_OP_SEQ_ALIGN costs at
 *            most that sum (the hit's path is one of the paths DTW minimises over), exactly where all sums are exact.
 * Tables and checks follow AEW_OP_SEQ_ALIGN: the two aew_align_seq_t tables (reused unchanged) and the pair table each
 * come as a device copy and a host copy; the launcher checks every host record before anything is launched, the kernels
 * repeat the checks on the device copies and leave a failing pair alone; no address is formed from an unchecked record.
 * The profile ranges [prof_base, prof_base + n) of the pairs must be disjoint - the caller's contract (prefix sums).
 * AEW_E_ARG: metric outside its values, D outside [1, AEW_ALIGN_MAX_D], n_pairs < 1 or > 2^24, n_a / n_b < 1, n_hits
 * outside [1, AEW_SEARCH_MAX_HITS], min_len or max_len negative, a threshold that is not finite, a NULL table or output
 * (prof_*, hits, hit_score, hit_steps, count, bad), a NULL feature buffer of n_feat > 0, n_feat outside [0, 2^50],
 * n_prof < 0, a sequence record AEW_OP_SEQ_ALIGN refuses, a pair with a / b outside its table, a negative band,
 * prof_base < 0 or prof_base + n > n_prof, an a of more than 64 frames without a workspace of the size stated at `ws`.
 * AEW_E_ALIGN: a table off 8 bytes, any other pointer off 4.  A refused call launches and writes nothing. */
typedef struct {
    int32_t a, b;                /* indices into the A-side / B-side sequence tables                            */
    int32_t band, pad_;          /* cells with j - i < band are dead (0: none); >= 0                            */
    int64_t prof_base;           /* first of the pair's n entries in the five profile arrays                    */
} aew_discover_pair_t;

typedef struct {
    int32_t metric, n_hits;      /* AEW_ALIGN_EUCLID / _SQEUCLID; 1 .. AEW_SEARCH_MAX_HITS      */
    int32_t D, n_pairs;
    int32_t min_len, max_len;    /* bounds on both spans of a hit; max_len 0: no upper limit    */
    float threshold;             /* the local distance at which a cell neither gains nor loses  */
    int32_t pad_;
    const aew_align_seq_t* seq_a;       /* device memory, n_a records                          */
    const aew_align_seq_t* seq_a_host;  /* the same records in host memory                     */
    const aew_align_seq_t* seq_b;
    const aew_align_seq_t* seq_b_host;
    const aew_discover_pair_t* pairs;   /* device memory, n_pairs records                      */
    const aew_discover_pair_t* pairs_host;
    int32_t n_a, n_b;
    const float* feat_a;         /* n_feat_a elements                                          */
    const float* feat_b;
    int64_t n_feat_a, n_feat_b;
    float* prof_score;           /* [n_prof]: E(i)                                             */
    int32_t* prof_end;           /* [n_prof]: the column the row's best alignment ends at      */
    int32_t* prof_row;           /* [n_prof]: the row it starts at                             */
    int32_t* prof_col;           /* [n_prof]: the column it starts at                          */
    int32_t* prof_steps;         /* [n_prof]: its cells                                        */
    int64_t n_prof;
    int32_t* hits;               /* [n_pairs][n_hits][4]: (a_start, a_end, b_start, b_end)     */
    float* hit_score;            /* [n_pairs][n_hits]                                          */
    int32_t* hit_steps;          /* [n_pairs][n_hits]                                          */
    int32_t* count;              /* [n_pairs]; between the two launches it carries the sweep's verdict on the pair */
    uint32_t* bad;               /* one device word, added to                                  */
    void* ws;                    /* boundary rows (H, S, origin row, origin column) of pairs with more than 64 A frames
                                    (optional): ws_bytes >= 16 * n_pairs * the longest B side among those pairs (the
                                    launcher takes that length from the host tables).  Contents are scratch.             */
    int64_t ws_bytes;
} aew_seq_discover_t;

/* ABX discriminability of a labelled item set (appended to ABI 28; AEW_OP_ABX_COUNT, aew_sizeof 58 / 59 - index 57 stays
 * unused, it answers -1): over an N x N distance matrix D (row = X, column = A or B; no symmetry is assumed) count, for
 * every X and every group of B items, the (A, B, X) triples and how many of them D gets wrong.  One launch, one
 * workgroup per X; nothing waits on another workgroup - no flag, no spin, no atomic, no floating-point sum.
 *
 * THE RULE (tests/abx_emulator.py restates it from the labels alone).  Item i carries a category and a speaker.  The
 * host sorts the items stably by (speaker, category): perm[x] = the item at sorted position x.  The G non-empty
 * (category, speaker) groups are contiguous ranges [lo, hi) of sorted positions; partner[cat * S + spk] = the group of
 * that (category index, speaker index), -1 where there is none.  D is read in place through the permutation:
 * d(x, j) = D[perm[x] * ld + perm[j]].
 *   cell     For a sorted position x in group (cX, sX) and a group g = (cB, sB), cell (x, g) is VALID when cB != cX, the
 *            speaker condition holds (WITHIN: sB == sX; ACROSS: sB != sX) and A = group(cX, sB) \ {x} is not empty.  A and
 *            B share a speaker; X has it too (WITHIN) or another one (ACROSS).
 *   counts   valid:   n[x][g] = |A| * |g|,  wrong2[x][g] = sum over a in A, b in g of w(d(x, a), d(x, b)),
 *                     w(p, q) = 2 if p > q; 0 if p < q; 1 otherwise (equal, or a NaN on either side);
 *            invalid: n[x][g] = wrong2[x][g] = 0.
 *            Rows of n / wrong2 are SORTED positions.  Every one of the N * G words of both outputs is written.  The sums
 *            are integers: no order of evaluation changes a bit.  wrong2 / (2 n) is the ABX error of the cell.
 * The launcher reads the HOST copies of the three tables before anything is launched; the kernel reads the device copies
 * and forms no address from a value it has not range-checked.  AEW_E_ARG: a mode outside the two, N outside
 * [1, AEW_ABX_MAX_N] (2 |A| |g| <= 2 (N / 2)^2 then fits 32 bits), G outside [1, N], C or S < 1, N * G > 2^27,
 * C * S > N * G (the launcher reads every word of the three host tables at every launch: that bounds it), ld < N, a NULL pointer, perm_host no permutation of [0, N), group ranges that do not tile [0, N) in
 * order (lo of the first 0, hi > lo, lo of the next = hi, hi of the last N), a category / speaker index outside
 * [0, C) / [0, S), a partner table that is not the inverse of the group table.  AEW_E_ALIGN: a pointer off 4 bytes.  A
 * refused call launches and writes nothing. */
#define AEW_ABX_WITHIN 0
#define AEW_ABX_ACROSS 1
#define AEW_ABX_MAX_N 16384
typedef struct {
    int32_t lo, hi;              /* sorted positions [lo, hi)                                   */
    int32_t cat, spk;            /* category index in [0, C), speaker index in [0, S)           */
} aew_abx_group_t;

typedef struct {
    int32_t mode;                /* AEW_ABX_WITHIN / _ACROSS                                    */
    int32_t N, G, C, S, pad_;
    int64_t ld;                  /* row pitch of dist in elements, >= N                         */
    const float* dist;           /* device memory, (N - 1) * ld + N elements; only read         */
    const int32_t* perm;         /* device memory, [N]                                          */
    const int32_t* perm_host;    /* the same words in host memory                               */
    const aew_abx_group_t* groups;       /* device memory, [G]                                  */
    const aew_abx_group_t* groups_host;
    const int32_t* partner;      /* device memory, [C][S]                                       */
    const int32_t* partner_host;
    uint32_t* n;                 /* [N][G]                                                      */
    uint32_t* wrong2;            /* [N][G]                                                      */
} aew_abx_count_t;

/* The op on the CPU: the same descriptor with HOST pointers everywhere (perm / groups / partner may be NULL, the _host
 * copies are read), the launcher's checks and return codes, the kernel's own definitions of w and of cell validity.
 * Host logic only (tests). */
int aew_abx_host(const aew_abx_count_t* p);

/* Reduce the chunk sums of a step to per-tensor norms (ABI 22).  One block of 256 threads per tensor: thread t adds the
 * contiguous run [t * per, (t + 1) * per) of the tensor's chunks, per = ceil(chunks / 256), ascending, then the fixed
 * wave / block tree of the gradient norm - separately for the two sums.
 *   finalize = 0 : sums[0][t] = sum (p_old - p_new)^2, sums[1][t] = sum p_old^2 - nothing else is written.
 *   finalize = 1 : the totals are the chunk sums (part may be NULL: none) + add_in[.][t] (optional); they go to sums
 *                  when that is given and out[0][t] = (float) sqrt(total 0) - the update norm, out[1][t] =
 *                  (float) sqrt(total 1) - the weight norm BEFORE the step, out[2][t] = out[0][t] / out[1][t], a plain fp32
 *                  division: a zero-initialised bias gives inf (or nan when it did not move), as the reference's loop.
 * Data parallel with sharded updates: launch 1 (finalize = 0) over what this rank updated, all-reduce of the 2 P fp64
 * words, launch 2 (finalize = 1, part = NULL, add_in = those words).
 * AEW_E_ARG: n_tensors < 1, first NULL, neither part nor add_in, finalize = 0 without part or sums, finalize = 1 without
 * out; AEW_E_ALIGN: part / add_in / sums not 8-byte, first / out not 4-byte aligned. */
typedef struct {
    const double* part;          /* device [n_chunks][2] (aew_uw_track_t.part)                                             */
    const int32_t* first;        /* device [n_tensors + 1]: first chunk of each tensor (aew_uw_chunks)                      */
    int32_t n_tensors;           /* P                                                                                     */
    int32_t finalize;
    const double* add_in;        /* optional device [2][P]                                                                 */
    double* sums;                /* device [2][P]                                                                          */
    float* out;                  /* device [3][P]: update norm, weight norm, ratio                                         */
} aew_update_ratio_t;

/* ---------------------------------------------------------------------------------------
 * Global gradient norm (ABI 21): what torch.nn.utils.clip_grad_norm_ computes over the parameters' .grad - here ONE
 * deterministic sum of squares over ranges of the flat fp32 gradient buffer, and a device-side clip coefficient that
 * aew_adam_t.clip multiplies in.  The host never reads the norm.
 *   launch   : one kernel; block j owns one chunk of AEW_GRAD_NORM_CHUNK floats of one range (ranges ascending, chunks
 *              ascending) - the grid depends on the range lengths only, never on the device
 *   sum      : fp64 from the first add; per thread four chains (the float4 components, float4 t, t + 256, ... of the
 *              chunk), a fixed butterfly inside the wave, waves ascending; one fp64 partial per block to `scratch`
 *   combine  : the block that draws the last ticket adds the partials - thread t the contiguous run
 *              [t * per, (t + 1) * per), per = ceil(blocks / 256), ascending, then the same wave / block tree - plus
 *              add_in[0], and is the only writer of sumsq / out.  No atomics on data: the bits do not depend on the
 *              order of arrival.
 *   finalize : norm = |grad_scale| * sqrt(total).  total inf / nan: out = {norm, 0, 1, skipped + 1}; else
 *              out = {norm, norm <= max_norm ? 1.0f (exactly) : max_norm / (norm + eps), 0, skipped}.
 * Data parallel with sharded gradients: launch 1 (finalize = 0) over this rank's shards, all-reduce of the one fp64
 * word `sumsq`, launch 2 (finalize = 1, add_in = that word) over what every rank holds.
 * AEW_E_ARG: n_ranges outside 1..8, n[i] < 0, a NULL pointer where one is needed, finalize without out;
 * AEW_E_ALIGN: x[i] not 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
#define AEW_GRAD_NORM_CHUNK 16384
#define AEW_GRAD_NORM_MAX_RANGES 8
typedef struct {
    const float* x[AEW_GRAD_NORM_MAX_RANGES];   /* 16-byte aligned (may be NULL where n[i] = 0)                           */
    int64_t n[AEW_GRAD_NORM_MAX_RANGES];        /* >= 0, any length                                                       */
    int32_t n_ranges;            /* 1..8                                                                                  */
    int32_t finalize;            /* 1: also write out[] from the total                                                    */
    const double* add_in;        /* optional device [1]: added to the sum (the other ranks' shards, after their all-reduce) */
    double* sumsq;               /* device [1]: sum over the ranges of x^2 (+ add_in[0])                                   */
    float max_norm, grad_scale, eps;   /* the norm is that of grad_scale * x; eps = 1e-6 is clip_grad_norm_'s               */
    int32_t pad_;
    float* out;                  /* [4]: total norm, clip coefficient, non-finite flag (0 / 1), steps skipped so far (a
                                    running count: zeroed by the caller once)                                             */
    double* scratch;             /* aew_grad_norm_size doubles                                                            */
    uint32_t* ticket;            /* aew_grad_norm_size words, zeroed once by the caller, left zero by every launch         */
    const uint32_t* guard;       /* optional, like aew_adam_t.guard: non-zero = the op leaves out[] untouched              */
} aew_grad_norm_t;
/* What scratch / ticket must hold.  Host logic only; the launcher uses the same arithmetic. */
int aew_grad_norm_size(const aew_grad_norm_t* g, int64_t* scratch_doubles, int32_t* tickets);

typedef struct { void* ptr; int64_t bytes; } aew_zero_t;

typedef struct {                 /* VAE reparameterisation (vae_bn.py:44-53) and its backward */
    const float* lin; int32_t lin_pitch;   /* [Q][2d pitch]: mu | log_sigma_sq               */
    const float* eps;                       /* [Q][d]                                        */
    int32_t Q, d, d_pitch;
    float* sample;                          /* [Q][d_pitch]                                  */
    float* kl_terms;                        /* fwd: [Q] per-row sum of 1+ls-mu^2-sigma^2     */
    const float* dsample; float kl_coef;    /* bwd: d(loss)/d(sample); d(loss)/d(KL)          */
    const float* kl_value; float free_nats; /* bwd: if kl_value != NULL the KL gradient is gated by
                                               [kl_value[0] >= free_nats] (torch.clamp backward)   */
    float* dlin;                            /* bwd: [Q][2d pitch]                            */
    int32_t backward;
    const float* kl_coef_dev;               /* if non-NULL, kl_coef is read from device memory at run time  */
    const float* gmul;                      /* optional device scalar: upstream d(L)/d(loss), multiplies kl_coef */
} aew_vae_t;

typedef struct {                 /* AE norm term (ae_bn.py:36-38): | ||ze|| - 1 | per row      */
    const float* ze; int32_t Q, d, d_pitch;
    float* term;                 /* fwd: [Q]                                                  */
    const float* dze_in; float coef; float* dze;  /* bwd: dze = dze_in + coef*sign*ze/||ze||   */
    int32_t backward;
    const float* gmul;           /* optional device scalar: upstream d(L)/d(loss), multiplies coef              */
} aew_ae_norm_t;

typedef struct {                 /* time-jitter indices on the device (jitter.py:13-33).  out[b][t] = t - 1 + X[b][t],
                                    X in {0,1,2}; X = 1 for t < 2.  mode 0 = what the reference does at HEAD:
                                    X iid with P = [p, 1-2p, p] (its conditional table is indexed [p1][p1], so the
                                    "no three in a row" rule never fires); mode 1 = the documented rule:
                                    P(X_t | X_t-2, X_t-1) = [p, s, p] except (2,1) -> [0, s/(p+s), p/(p+s)].
                                    Randomness: counter-based, u(b,t) = mix64(seed, step, b, t) / 2^53 in [0,1);
                                    X = (u >= c0) + (u >= c1) on the cumulative table (oracle/jitter_rng.py is the
                                    same arithmetic in numpy: bit-identical output).                                  */
    int64_t* out; int32_t out_pitch;
    int32_t B, n;
    float p;
    int32_t mode;
    uint64_t seed, step;
} aew_jitter_t;

/* ---------------------------------------------------------------------------------------
 * Device-resident training corpus (ABI 28): the batch's windows are cut out of a corpus that lives in device memory, in
 * ONE op, with no host work and no host synchronisation (the reference: data.py SliceDataset / LoopingRandomSampler /
 * TrackerDataset, a Python loop per item under a DataLoader).  The op reads how many items this rank has consumed from
 * a DEVICE counter, so a captured graph that holds it yields the next batch at every replay.
 *
 *   snd      the corpus: n_snd elements of snd_bytes = 1 (uint8), 2 (int16) or 4 (int32) bytes (data.py:35-40).
 *            CONTRACT: the base is 16-byte aligned and at least 16 bytes are readable past the last element.
 *   starts   int64 [N], voices int32 [N]: the reference's in_start table (slice start in elements, speaker), its order.
 *   order    int32 [2][n_order]: the permutation of this rank's slice list range(rank, N, num_replicas) for two
 *            consecutive sampler epochs; epoch e reads row e & 1 (a batch may straddle two epochs).
 *            n_order = len(range(rank, N, num_replicas)) = (N - rank + num_replicas - 1) / num_replicas.
 *   counter  uint64 [1]: items this rank has consumed since the start.
 *
 * With t0 = *counter, R = num_replicas, for batch item b < B:
 *   j = t0 + b;  e = j / n_order;  p = j % n_order;  i = rank + R * order[e & 1][p]
 *   wav[b * wav_pitch + k] = (float)snd[starts[i] + k], k < slice_size     (data.py:229; int32 rounds to nearest even;
 *                                                        columns slice_size..wav_pitch-1 are NOT written)
 *   voice[b] = voices[i];  index[b] = i
 * and with P = ceil(N / R), t = t0 + B:
 *   position[0] = t / P;  position[1] = (t % P) * R      (what TrackerDataset reports for the LAST item of the batch:
 *                                                        step += R per item, at step >= N: epoch += 1, step = 0)
 * After every block has read the counter - a second launch of one thread inside the same launcher, no grid-wide wait -
 * *counter = t0 + B when advance != 0 (advance == 0: the same batch again at the next launch).
 * A table entry that would leave the corpus (an order value outside [0, n_order), i >= N, starts[i] < 0 or
 * starts[i] + slice_size > n_snd) is not followed: that row of wav reads as zeros, voice[b] = -1, index[b] = -1.
 *
 * Kernel: grid (ceil(slice_size / (4096 / snd_bytes)), B), 256 threads; a lane converts 16 source bytes (16 / 8 / 4
 * elements) and writes them with 16-byte stores.  Slice starts have every alignment: the lane reads the two ALIGNED
 * 16-byte quantities that hold its 16 bytes and realigns them in registers, so the stores are aligned to the row of wav
 * and there is no element-wise head; the slice_size % (16 / snd_bytes) elements at the end are read and written one
 * by one.  Nothing below snd is read and nothing beyond the 16 bytes of slack the contract grants.
 *
 * Before any launch: AEW_E_ARG for B < 1 or B > 65535 (grid rows), slice_size <= 0, snd_bytes outside {1, 2, 4}, num_replicas < 1, rank outside
 * [0, num_replicas), N < 1, n_order < B, n_order != len(range(rank, N, num_replicas)), n_snd < slice_size,
 * wav_pitch < slice_size or not a multiple of 4, a NULL pointer; then AEW_E_ALIGN for snd or wav not 16-byte aligned,
 * starts / counter / voice / position not 8-byte aligned, voices / order / index not 4-byte aligned. */
typedef struct {
    const void* snd; int64_t n_snd; int32_t snd_bytes; int32_t B;
    const int64_t* starts; const int32_t* voices; int64_t N;
    const int32_t* order; int32_t n_order; int32_t num_replicas; int32_t rank; int32_t advance;
    uint64_t* counter;
    int32_t slice_size; int32_t wav_pitch;
    float* wav; int64_t* voice; int32_t* index; int64_t* position;
} aew_window_gather_t;

/* The index arithmetic of aew_window_gather_t for item b of the batch that starts at counter value t0, from the same
 * helper the kernel calls: *epoch = e, *p = p, (*pos_epoch, *pos_step) = position.  Host-only, no device needed.
 * AEW_E_ARG for a NULL output, B < 1, b outside [0, B), N < 1, n_order < 1, R < 1, rank outside [0, R), or an epoch
 * that does not fit an int. */
int aew_corpus_locate(uint64_t t0, int b, int B, int64_t N, int n_order, int R, int rank, int* epoch, int* p,
                      int64_t* pos_epoch, int64_t* pos_step);

/* ---------------------------------------------------------------------------------------
 * Gradient noise statistics (ABI 28, appended; aew_sizeof 22 / 23): what the reference's grad_analysis.py computes with six elementwise torch kernels per
 * tensor and batch (mu_s_incr) and one kthvalue + .item() per tensor and quantile (quantiles) - here one launch per gradient
 * sample over three flat fp32 buffers with the offsets of the parameters, and one op for every quantile of every tensor.
 *
 * AEW_OP_GRAD_WELFORD folds the gradient sample g into the running mean mu and the running sum of squared deviations s.
 * Per element (grad_analysis.py:32-39), in round-to-nearest fp32 operations that the compiler may not contract, the
 * division a true fp32 division - a numpy fp32 restatement gives the same bits:
 *     first != 0 :  mu = g;  s = 0                                  (mu / s are not read)
 *     first == 0 :  d = g - mu;  mu' = mu + d / divisor;  s' = s + d * (g - mu')
 * float4 loads and stores with a scalar tail; every element of [0, n) is updated, the pad elements behind a tensor like
 * any other (as Adam updates them).  `divisor` is the host's: the reference passes its loop index, the textbook the count.
 * part != NULL: the launch runs one block per chunk of the chunk table (aew_uw_chunks; chunks = device copy, chunks_host =
 * host copy, n_chunks records), exactly as the tracked Adam launch does, and also WRITES (plain stores: no two blocks
 * share a chunk)
 *     part[chunk] = {sum s', sum mu'^2}   over the chunk's own elements (pad elements enter no sum)
 * in fp64 in the order aew_uw_track_t documents: per thread one chain per sum (the thread's float4 rounds ascending,
 * components ascending), a fixed butterfly inside the wave, waves ascending.  AEW_OP_UPDATE_RATIO with finalize = 0 then
 * yields the per-tensor sums [2][P].  The chunks and the pads behind them must cover [0, n) without a gap (AEW_E_ARG), so
 * the mu / s bits do not depend on whether part is set - the two launches share one per-element device function.
 * Before any launch - AEW_E_ARG: n < 0, a NULL g / mu / s with n > 0, first outside {0, 1}, divisor not > 0 with
 * first == 0, buffers that overlap, with part a NULL / empty / non-covering chunk table; AEW_E_ALIGN: g, mu, s or part not
 * 16-byte aligned.  n == 0 is a no-op. */
typedef struct {
    const float* g; float* mu; float* s;
    int64_t n;
    int32_t first;               /* 1: the first sample (mu = g, s = 0)                                                    */
    float divisor;
    const aew_uw_chunk_t* chunks;        /* device copy of the chunk table (with part)                                     */
    const aew_uw_chunk_t* chunks_host;   /* host copy: the launcher checks the coverage of [0, n) in it                     */
    int64_t n_chunks;
    double* part;                /* optional device [n_chunks][2]                                                          */
} aew_grad_welford_t;

/* AEW_OP_SEG_SELECT: the exact k-th smallest element of every tensor of the flat buffer s, for Q <= AEW_SELECT_MAX_Q ranks
 * per tensor at once, through the chunk table (a chunk's `tensor` names the row of k / out it belongs to; tensors of
 * length 0 have no chunk).  The reference takes kthvalue(k) of sqrt(s / n_batch) (grad_analysis.py:42-50, 82-83); both are
 * monotone, so the op selects on s and transforms only the winner.
 *   order key : the fp32 bit pattern for s >= 0 (-0 counts as +0), 0xFFFFFFFF for s < 0 or NaN - the reference's sqrt makes
 *               those NaN and kthvalue ranks NaN last.  aew_select_key is the function the kernels call.  (The key is that
 *               of s alone: a negative s so small that s / denom underflows to -0 is -0 to the reference, NaN here.)
 *   ranks     : k[t][q], device int32, 1-based, 1 <= k <= length of tensor t.
 *   out[t][q] : with v = the value whose key is the k-th smallest:  raw != 0: v;  raw == 0: sqrt(v / denom), a true fp32
 *               division and a correctly rounded root; NaN for the NaN key (raw or not), for a tensor of length 0 and for
 *               a rank outside 1 .. length.
 *   method    : radix select, four passes of 8 key bits.  Pass kernel: one block per chunk, an LDS histogram of the next 8
 *               bits per live (tensor, rank) prefix (ranks that share a prefix share a histogram), non-zero bins added to
 *               hist[t][q][256] with integer atomics.  Pick kernel: one block per tensor finds the bin that holds the
 *               rank, narrows the prefix, reduces the rank, clears the bins.  Integer atomics only: exact in any order.
 *   scratch   : aew_seg_select_size bytes, 16-byte aligned; the op zeroes what it needs itself, so two calls in a row give
 *               the same bits without host work in between.
 * Before any launch - AEW_E_ARG: Q outside 1..8, n_tensors < 1, a NULL k / out / scratch, a NULL s / chunks with
 * n_chunks > 0, raw outside {0, 1}, denom not > 0 with raw == 0; AEW_E_ALIGN: s or scratch not 16-byte, chunks not 8-byte,
 * k or out not 4-byte aligned. */
#define AEW_SELECT_MAX_Q 8
typedef struct {
    const float* s;
    const aew_uw_chunk_t* chunks;        /* device                                                                         */
    int64_t n_chunks;
    int32_t n_tensors;           /* P                                                                                      */
    int32_t Q;                   /* 1 .. AEW_SELECT_MAX_Q ranks per tensor                                                  */
    const int32_t* k;            /* device [P][Q]                                                                          */
    float* out;                  /* device [P][Q]                                                                          */
    float denom;
    int32_t raw;
    void* scratch;
} aew_seg_select_t;
/* Bytes of scratch the op needs (P and Q are read from *p).  Host logic only. */
int aew_seg_select_size(const aew_seg_select_t* p, int64_t* bytes);
/* *key = the order key of the value with fp32 bit pattern `bits`: the very function the kernels call.  Host-only, no
 * device.  AEW_E_ARG for a NULL key. */
int aew_select_key(uint32_t bits, uint32_t* key);

/* ---------------------------------------------------------------------------------------
 * Chained NT launch (ABI 19): a run of DEPENDENT bf16 NT ops - the gated stack's G1 / G2 pairs (wavenet.py:100-109,
 * 354-357: the layer loop) or its backward's dz / dx pairs - as ONE kernel launch.  The tiles of all stages form one
 * grid in stage order; a tile of stage s starts once the tiles of earlier stages that produce the rows it reads have
 * published them (tile-granular hand-off through device-scope counters), so a stage's first tiles run in the slots
 * its predecessor's last tiles leave free and the launch pays the fill / drain of a dependent launch once instead of
 * once per op (profiles/r04_notes.md 13: ~10 us each, 84 times per step).
 *   producer tile : out0 stored write-through (sc1), every wave drains its stores, one lane adds 1 to the counter of
 *                   its (stage, batch element, row tile) - device scope
 *   consumer tile : one wave polls the counters of the producer row tiles it reads (relaxed device-scope loads, bounded
 *                   spin), workgroup barrier, then its activation and epilogue operands with device-scope (sc1) loads
 * No assumption on workgroup -> XCD placement.  The bounded spin relies on workgroups being dispatched in index
 * order (every producer of a resident tile has been dispatched): a wait that times out sets *err and the tile runs on.
 * Same kernel bodies, tile shape (256 x 128) and summation order as the stand-alone launches of the default shape
 * (k_gemm_nt_bf16<.., 4> / k_gemm_nt_bf16_win), so results are bit-identical to the serial plan.
 *
 * In a plan the chain op sits IN FRONT of its n_ops stage ops (plain AEW_OP_GEMM_NT records).  When chaining is on
 * (aew_tuning_t.nt_chain, default 1) and the call is not in per-op timing mode, aew_run_plan launches the chain and
 * skips the n_ops records; otherwise the chain op does nothing and the records run as stand-alone launches (what the
 * timing pass and the CPU plan interpreter execute) - the two forms read and write the same buffers.
 * The stage table is built on the HOST by aew_nt_chain_build from the same n_ops descriptors (dependencies derived
 * from the segment / view records; anything it cannot prove safe is refused) and uploaded by the caller.
 * ------------------------------------------------------------------------------------- */
#define AEW_CHAIN_MAXDEP 3
typedef struct {
    int32_t cnt_base;            /* first counter of the producer stage                                       */
    int32_t n_mt;                /* its row tiles per batch element                                           */
    int32_t need;                /* arrivals per row tile = its N tiles                                       */
    int32_t d_lo, d_hi;          /* consumer rows [m_first, m_last] read producer rows [m_first + d_lo, m_last + d_hi] ... */
    int32_t c_lo, c_hi;          /* ... clipped to [c_lo, c_hi] (rows the producer writes and the consumer can read) */
    int32_t bm;                  /* producer tile rows                                                        */
} aew_chain_dep_t;

typedef struct {
    aew_gemm_nt_t g;
    int32_t kind;                /* kernel body: 0 plain K loop, 1 one-window (d <= 16), 2 one-window (d <= 64)   */
    int32_t first_block;         /* multiple of 8                                                             */
    int32_t n_blocks;
    int32_t n_mt, n_nt;
    int32_t cnt_base;            /* counters [batch][n_mt] of this stage                                      */
    int32_t publish;             /* a later stage waits for this one                                          */
    int32_t n_deps;
    aew_chain_dep_t dep[AEW_CHAIN_MAXDEP];
} aew_nt_stage_t;

typedef struct {
    const aew_nt_stage_t* stages;    /* device                                                                */
    const uint16_t* block_stage;     /* device: stage of blocks [8 i, 8 i + 8)                                */
    uint32_t* counters;              /* device, 16-byte aligned, n_counters + 8 words rounded up to 16 bytes, zeroed by the launch:
                                        the counters, then [n_counters] timeout flag (stage + 1 of a wait that gave up),
                                        [+1] tiles that found a producer unfinished, [+2] the longest wait in polls */
    int32_t n_stages, n_blocks, n_counters;
    int32_t set;                     /* 0: GATED / STORE bodies (forward), 1: DFG / STORE bodies (backward)    */
    int32_t n_ops;                   /* stage ops that follow this op in the plan                              */
    int32_t spin_max;                /* polls before a wait gives up (0: default 1 << 18)                      */
    int32_t flags;                   /* 4 = consumers also issue an agent-scope acquire fence (A/B; the sc1 loads make it redundant);
                                        2 = the caller zeroes `counters` itself before the launch (a plan with several chains:
                                        one AEW_OP_ZERO for all of them) */
    int32_t built_window;            /* ABI 20: aew_tuning_t.nt_window the stage table was built under (it decides which stages
                                        take the one-window body, i.e. their summation order).  A launch under a record that
                                        disagrees runs the stage ops one by one instead - the chain never executes another
                                        kernel than the serial plan would                                                */
    uint32_t* sticky;                /* ABI 20, optional device word that NO launch clears: a wait that gives up also stores
                                        (stage + 1) here (atomic max).  aew_adam_t.guard / aew_vq_ema_t.guard read it.    */
} aew_nt_chain_t;

/* Host logic only.  descs[0..n): the stage descriptors in execution order.  Fills stages_out[n] (host memory; `g` copied
 * in), block_stage_out[cap_blocks / 8] and *n_blocks / *n_counters / *set.  force != 0: chain also launches the stand-alone
 * launcher would run on its small-launch shapes (tests).  Returns 0, AEW_E_UNSUP if the run cannot be chained (a
 * descriptor outside the default bf16 shapes, a dependency the builder cannot express, a buffer reused inside the run),
 * AEW_E_ARG on malformed input. */
int aew_nt_chain_build(const aew_gemm_nt_t* descs, int n, aew_nt_stage_t* stages_out, uint16_t* block_stage_out,
                       int cap_blocks, int* n_blocks, int* n_counters, int* set, int force);
/* Producer row tiles consumer tile (first row m0 of the 256-row tile) of `stage` waits for through dependency `dep`:
 * [*t_lo, *t_hi] (empty if *t_lo > *t_hi).  The kernel uses the same arithmetic; exported for tests. */
int aew_nt_chain_dep_tiles(const aew_nt_stage_t* stage, int dep, int m0, int* t_lo, int* t_hi);
/* aew_nt_stage_t.kind bit of a stage on 128-row tiles (aew_nt_chain_build_bm, below): body kind = kind & 3, and m0 above
 * is then the first row of a 128-row tile.  aew_chain_dep_t.bm is the PRODUCER's height. */
#define AEW_CHAIN_KIND_128 4

/* Split-K hint for a small bf16 launch (aew_gemm_nt_t.k_split): *k_split = the largest S in 2..8 the launcher would honour
 * for g under the calling thread's tuning record with S * blocks <= target_blocks and at least four 64-channel K tiles per
 * range, or 1 (leave g alone); *ws_bytes / *n_tickets = what ksplit_ws / ksplit_tickets must then hold.  Host-only.   */
int aew_gemm_nt_small_split(const aew_gemm_nt_t* g, int target_blocks, int* k_split, int64_t* ws_bytes, int* n_tickets);

/* ---------------------------------------------------------------------------------------
 * plan
 * ------------------------------------------------------------------------------------- */
enum {
    AEW_OP_GEMM_NT = 1, AEW_OP_GEMM_TN, AEW_OP_COPY_TABLE, AEW_OP_VQ_NEAREST, AEW_OP_VQ_STATS,
    AEW_OP_VQ_EMA, AEW_OP_VQ_BWD, AEW_OP_LC_GATHER, AEW_OP_LC_SCATTER, AEW_OP_SPK_BIAS,
    AEW_OP_SPK_BWD, AEW_OP_BASE_GATHER, AEW_OP_SOFTMAX_NLL, AEW_OP_COLSUM, AEW_OP_REDUCE,
    AEW_OP_ADAM, AEW_OP_ZERO, AEW_OP_VAE, AEW_OP_AE_NORM, AEW_OP_JITTER, AEW_OP_VQ_DIAG, AEW_OP_MFCC,
    AEW_OP_MOMENTS, AEW_OP_GEMM_TN_GROUP, AEW_OP_NT_CHAIN, AEW_OP_GRAD_NORM, AEW_OP_UPDATE_RATIO,
    AEW_OP_SWAP, AEW_OP_VQ_RESTART, AEW_OP_EVAL_ACC, AEW_OP_WINDOW_GATHER, AEW_OP_GRAD_WELFORD, AEW_OP_SEG_SELECT,
    AEW_OP_ACCUM, AEW_OP_CODE_LOOKUP, AEW_OP_CODE_RUNS, AEW_OP_ADAM_GROUPS,
    AEW_OP_EVAL_GROUPS, AEW_OP_MEL_TILE, AEW_OP_CODE_STITCH, AEW_OP_CODE_TILE, AEW_OP_COND_STITCH,
    AEW_OP_WAV_TILE, AEW_OP_NLL_STITCH, AEW_OP_SCORE_REDUCE, AEW_OP_SEQ_ALIGN,
    AEW_OP_FRAME_STITCH, AEW_OP_CODE_SEGMENT, AEW_OP_SEQ_SEARCH, AEW_OP_ABX_COUNT, AEW_OP_SEQ_DISCOVER
};

/* Lanes.  A plan is a sequential program; `lane` lets the caller mark ops that are OFF the
 * critical chain (weight gradients, bias column sums, weight packing) so that they execute on side
 * HIP streams / parallel hipGraph branches and fill the tails of the chain's kernels:
 *   lane 0 (main)      runs after the preceding lane-0 ops; it waits for preceding side ops only if
 *                      `join` != 0.  The end of the plan is an implicit join.
 *   lane k = 1..5      runs after ALL lane-0 ops that precede it in the plan and after the preceding ops
 *                      of the SAME lane; with `join` != 0 also after the preceding ops of every other side
 *                      lane.  Ops on different side lanes are otherwise unordered (they may run concurrently).
 * Any serial execution in plan order is a valid schedule (that is what the timing mode and
 * aew_set_lanes(0) do), so a lane assignment is correct iff it respects every true dependency. */
typedef struct {
    int32_t kind;
    int32_t tag;                 /* caller-defined label, reported by the timing interface    */
    int32_t lane;                /* 0 main, 1..5 side lanes                                    */
    int32_t join;                /* 1: wait for the preceding ops of all (other) side lanes first;
                                    10+k (lane-0 ops): wait for the preceding ops of side lane k only */
    union {
        aew_gemm_nt_t nt; aew_gemm_tn_t tn; aew_copy_table_t copy; aew_vq_nearest_t vqn;
        aew_vq_stats_t vqs; aew_vq_ema_t vqe; aew_vq_bwd_t vqb; aew_lc_gather_t lcg;
        aew_lc_scatter_t lcs; aew_spk_bias_t spk; aew_spk_bwd_t spkb; aew_base_gather_t base;
        aew_softmax_nll_t sm; aew_colsum_t cs; aew_reduce_t red; aew_adam_t adam; aew_zero_t zero;
        aew_vae_t vae; aew_ae_norm_t aen; aew_jitter_t jit; aew_vq_diag_t diag; aew_mfcc_t mfcc;
        aew_moments_t mom; aew_gemm_tn_group_t tng; aew_nt_chain_t chain; aew_grad_norm_t gnorm; aew_update_ratio_t ratio;
        aew_swap_t swap; aew_vq_restart_t vqr; aew_eval_acc_t eva; aew_window_gather_t wgat;
        aew_grad_welford_t gwel; aew_seg_select_t ssel; aew_accum_t accum;
        aew_code_lookup_t clk; aew_code_runs_t crun; aew_adam_grouped_t adamg;
        aew_eval_groups_t evg; aew_mel_tile_t mtile; aew_code_stitch_t cstitch;
        aew_code_tile_t ctile; aew_cond_stitch_t cndst;
        aew_wav_tile_t wtile; aew_nll_stitch_t nllst; aew_score_reduce_t sred; aew_seq_align_t align;
        aew_frame_stitch_t fstitch; aew_code_segment_t cseg; aew_seq_search_t search;
        aew_abx_count_t abx; aew_seq_discover_t discover;
    } u;
} aew_op_t;

/* Library / build identification. */
int aew_abi_version(void);
/* sizeof(aew_op_t) etc. so the binding can verify its struct mirrors. */
int aew_sizeof(int which);      /* 0 op, 1 gemm_nt, 2 gemm_tn, 3 seg, 4 view, 5 copy_rec, 6 actor, 7 sampler, 8 tuning, 9 nt_stage, 10 nt_chain, 11 adam, 12 grad_norm, 13 uw_chunk, 14 uw_track, 15 update_ratio, 16 nt_pick, 17 swap, 18 vq_restart, 19 tn_pick, 20 eval_acc, 21 window_gather, 22 grad_welford, 23 seg_select, 25 accum, 27 code_lookup, 28 code_runs, 29 adam_tensor, 30 adam_groups, 31 adam_grouped, 32 eval_groups, 34 utt_row, 35 mel_tile, 36 code_stitch, 37 cond_row, 38 code_tile, 39 cond_stitch, 41 draw, 42 score_row, 43 wav_tile, 44 nll_stitch, 45 score_reduce, 47 align_seq, 48 align_pair, 49 seq_align, 51 seg_utt, 52 frame_stitch, 53 code_segment, 55 search_pair, 56 seq_search, 58 abx_group, 59 abx_count, 61 discover_pair, 62 seq_discover (24, 26, 33, 40, 46, 50, 54, 57 and 60 are unused: -1, like every index behind the last) */

/* Execute ops[0..n) in order on `stream` (a hipStream_t).  Returns at the first error and
 * writes the failing index to *fail_index if non-NULL. */
int aew_run_plan(const aew_op_t* ops, int n, void* stream, int* fail_index);

/* hipGraph form of a plan: capture once (on a private stream; pointers and scalars inside the
 * ops are frozen), replay with one launch per step on any stream.  `exec` is an opaque handle. */
int aew_graph_capture(const aew_op_t* ops, int n, void** exec, int* fail_index);
int aew_graph_launch(void* exec, void* stream);
int aew_graph_destroy(void* exec);

/* Per-op timing: while enabled, aew_run_plan brackets every op with HIP events on `stream`;
 * aew_timing_read synchronises the stream and returns elapsed ms per executed op (in
 * execution order since the last enable) and its tag.  aew_timing_enable(1): every op is its own launch (the stage ops of
 * an AEW_OP_NT_CHAIN run one by one, the chain op itself is an empty interval); (2): a chain runs as the ONE launch it
 * is in the untimed plan and carries the time, its stage ops are empty intervals.  One interval per op either way. */
/* =======================================================================================
 * Tuning context (ABI 17).  Every aew_set_* switch below edits ONE process-wide instance of this record; a caller that
 * wants its own settings - two engines with different shapes in one process, an A/B that must not leak - passes a record
 * to aew_run_plan_tuned / aew_graph_capture_tuned instead, which applies to that call only (thread-local for its duration;
 * a captured graph keeps the settings it was captured under).  aew_tuning_default fills in the library defaults,
 * aew_tuning_get the current process-wide values.  None of the fields changes a result beyond what the individual
 * switch documents (bit-identical shapes; the one-window kernel's summation order).
 * The tn_* fields that decide a TN op's split-K plan (tn_fold_rows, tn_target_blocks, tn_small_tiles, tn_small_target,
 * tn_big, tn_big_target) are read from the PROCESS-WIDE record also inside a *_tuned call: plan construction
 * (aew_tn_slabs) sized the slab buffers under it, and a launch must write exactly those slabs.  Set them with
 * aew_tuning_set / the aew_set_tn_* calls BEFORE building a plan.
 * ======================================================================================= */
typedef struct {
    int32_t nt_wave_rows;
    int32_t nt_pipe;
    int32_t nt_rows192;
    int32_t nt_small_tiles;
    int32_t nt_small_n64;
    int32_t nt_small_w8;
    int32_t nt_small_deep;
    int32_t nt_window;
    int32_t nt_mem128;
    int32_t nt_deep;
    int32_t nf_loaders;
    int32_t nf_deep;
    int32_t fn_enable;
    int32_t fn_ring3;
    int32_t tn_safe;
    int32_t tn_big;
    int32_t tn_big_target;
    int32_t tn_fold_rows;
    int32_t tn_target_blocks;
    int32_t tn_small_tiles;
    int32_t tn_small_target;
    int32_t lanes;
    int32_t tn_cursor_epoch;     /* ABI 18: aew_set_tn_cursor */
    int32_t tn_cursor_slack;
    int32_t nt_chain;            /* ABI 19: 1 (default) AEW_OP_NT_CHAIN ops launch their chain, 0 their stage ops run one by one */
    int32_t deterministic;       /* ABI 20: 1 (default) every sum of the training step has ONE order: column sums and the
                                    speaker-embedding gradient use their ticketed forms where the descriptor carries
                                    det_scratch / det_tickets; 0 = fp32 atomics (A/B of the cost).  One exception: the
                                    bias / projection gradients of aew_spk_bwd_t are order-fixed only up to 32 batch
                                    elements (beyond, their 16-element chunk sums meet in fp32 atomics in either mode;
                                    the speaker-embedding sums stay ticketed for every B)                              */
    int32_t tn_mfma32;           /* ABI 20: 1 = the grouped weight-gradient launch (tile = 128, no cursor) on v_mfma_f32_32x32x16_bf16:
                                    half the MFMA instructions per stage; same products, 16-row instead of 32-row partial sums
                                    (equal to fp32 rounding, not bit for bit, to the 16 x 16 x 32 form).  0 (default)            */
    int32_t reserved_[5];
} aew_tuning_t;
int aew_tuning_default(aew_tuning_t* out);
int aew_tuning_get(aew_tuning_t* out);
int aew_tuning_set(const aew_tuning_t* in);          /* replaces the process-wide instance (values are clamped like the setters') */
int aew_run_plan_tuned(const aew_op_t* ops, int n, void* stream, int* fail_index, const aew_tuning_t* tuning);
int aew_graph_capture_tuned(const aew_op_t* ops, int n, void** exec_out, int* fail_index, const aew_tuning_t* tuning);
/* aew_nt_chain_build under `tuning` (NULL: the process-wide record) - pass the record the plan will RUN under (aew_run_plan_tuned) and
 * store its nt_window in aew_nt_chain_t.built_window. */
int aew_nt_chain_build_tuned(const aew_gemm_nt_t* descs, int n, aew_nt_stage_t* stages_out, uint16_t* block_stage_out,
                             int cap_blocks, int* n_blocks, int* n_counters, int* set, int force, const aew_tuning_t* tuning);
/* ... and with a row-tile height per stage: stage_bm[n], each 256 or 128 (NULL: 256 throughout, the call above).  A stage on
 * 128-row tiles carries kind + AEW_CHAIN_KIND_128 and runs the same K order on half-height tiles of the same eight waves, so
 * its results are the 256-row stage's bit for bit.  128 is for the stages of the backward set (DFG, and STORE next to them):
 * AEW_E_UNSUP for a run that would launch the forward set with one.  cap_blocks counts every stage's tiles at its own height. */
int aew_nt_chain_build_bm(const aew_gemm_nt_t* descs, int n, aew_nt_stage_t* stages_out, uint16_t* block_stage_out,
                          int cap_blocks, int* n_blocks, int* n_counters, int* set, int force, const aew_tuning_t* tuning,
                          const int32_t* stage_bm);

/* Box fingerprint (measurement aid): sustained rate of THIS device on a pure bf16 MFMA loop (out[0], TFLOP/s) and on a
 * device-to-device copy of copy_bytes (out[1], TB/s read + written), HIP events on `stream`.  scratch: device memory,
 * 16-byte aligned, >= 2 * copy_bytes (>= 1 MiB each; contents are overwritten).  Synchronises the stream. */
int aew_probe_box(void* scratch, int64_t scratch_bytes, int64_t copy_bytes, void* stream, float* out);

int aew_timing_enable(int on);
int aew_timing_read(float* ms, int32_t* tags, int capacity, int* count);

/* Tile / wave shape of the bf16 NT kernel.  Same results bit for bit; tuning / A-B aid (profiles/r01_notes.md).
 *   64  (default) 256x128 tiles, 8 waves of 64x64, K tiles of 32; per launch the 192x128 or 64x128 shapes where
 *       the cost model prefers them (aew_set_nt_rows192, aew_set_nt_small_tiles)
 *   128 256x128 tiles, 4 waves of 128x64          256 256x256 tiles, 8 waves of 128x64 (N_pad % 256 == 0)
 *   0   128x128 tiles with K tiles of 64          1   256x128 tiles with K tiles of 64 */
int aew_set_nt_wave_rows(int rows);
/* Shapes 128 / 256 only: 1 (default) the register-double-buffered loop, 2 K tiles of 64, 0 the plain loop. */
int aew_set_nt_pipe(int on);
/* impl = 2 descriptors (full-N kernels, aew_fn.hip): 1 (default) use them where the shape is covered, 0 run every
 * impl = 2 descriptor on the tiled kernels instead (A/B and bisecting aid; same results). */
int aew_set_fn(int on);
int aew_set_fn_ring3(int min_k_tiles);   /* plain full-N GEMMs of >= this many 64-channel K tiles take the three-stage
                                            operand ring (default 16; 0 = never).  Same results either way.       */
/* Which kernel a GEMM_NT descriptor dispatches to under the current settings: 0 k_gemm_nt_bf16 (256- / 192-row tiles),
 * 1 k_gemm_nt_bf16_p64 (64-row tiles, small launches), 2 k_fn, 3 k_gemm_nt_f32, 4 the scalar check kernel, 5 an A/B
 * shape, 6 the one-window kernel - or the error code the launch would return for a descriptor it refuses.  Measurement
 * aid: lets a caller group per-op times by kernel the way a rocprofv3 kernel trace does. */
int aew_nt_kernel(const aew_gemm_nt_t* g);
/* ABI 23, test and measurement aid: everything the launcher decides for g under the current settings, without launching.
 * Returns what the launch would return for a malformed / unsupported descriptor (*out untouched), else 0 and
 *   kernel      the aew_nt_kernel code (6: the one-window kernel)
 *   variant     row of the library's table of NT kernel instantiations (-1: a full-N kernel, chosen by its own launcher:
 *               name "k_fn", lds_bytes 0)
 *   bm, bn      output tile of that row; threads, lds_bytes: its block and dynamic LDS
 *   grid        grid.x of the launch (k_split copies of the tile grid)
 *   k_split     K ranges the launch runs (1 unless the shape honours aew_gemm_nt_t.k_split)
 *   dwp         extra 16-row window pieces of the one-window kernel (1 | 4), 0 for every other kernel
 *   name        the instantiation as written in the table, blanks removed: "k_gemm_nt_bf16<0,false,4>"
 * Of a fused gated layer (W2) that runs unfused it describes the first launch, the GATED one. */
typedef struct {
    int32_t kernel, variant, bm, bn, threads, lds_bytes, grid, k_split, dwp;
    char name[96];
} aew_nt_pick_t;
int aew_nt_pick(const aew_gemm_nt_t* g, aew_nt_pick_t* out);
/* Default shape only: memory-bound plain launches (DFG epilogue, or K_total <= 256: wavenet.py:103-109 and the backward of
 * :100-102) as 128-row tiles - 0 the 256- / 192-row tiles, 1 128 x 128 tiles with K tiles of 32 (4 waves, three blocks
 * per CU), 2 128 x 128 tiles with K tiles of 64 (two blocks per CU).  Bit-identical results. */
int aew_set_nt_mem128(int mode);
/* Default shape only (A/B): deep operand rings at one block per CU - 1 256 x 128 tiles on a 6-stage ring, 2 256 x 256
 * tiles (8 waves of 128 x 64) on a 5-stage ring where N_pad % 256 == 0 and as 1 elsewhere, 3 as 2 with every other launch
 * on its default kernel.  0 (default) off.  Same results as the kernel each launch replaces, up to the order in which the
 * one-window kernel interleaves its taps. */
int aew_set_nt_deep(int mode);
/* Default shape only: bf16 NT launches of <= n 256x128 tiles use 64x128 tiles instead (0 = never). */
int aew_set_nt_small_tiles(int n);
/* ... and of those, launches of <= max_blocks blocks (default 256: one block per CU) run a 5-stage operand ring
 * instead of 2 stages: their K loop is DMA latency, not MFMA (0 = never; same results). */
int aew_set_nt_small_n64(int max_blocks);   /* launches of <= this many 64 x 128 blocks run as 64 x 64 tiles (twice the
                                               blocks, 2/3 of the operand bytes per block; default 256, 0 = never)  */
int aew_set_nt_small_deep(int max_blocks);
/* ... as 8 waves of 16 rows x 64 channels (default) or 2 waves of 64 x 64 per block (A/B; same results). */
int aew_set_nt_small_waves(int waves);
/* fp32 NT kernel: launches of <= max_blocks blocks (default 256 = one per CU) run with a 12-14 stage operand ring
 * (the whole LDS of the CU; 16-row tiles if that fits the limit, else 32-row tiles), larger ones with 5 stages and
 * three blocks per CU.  0 = always the 5-stage shape.  The chains themselves - one per output, k ascending - do not
 * change (bit-identical results). */
int aew_set_nf_deep(int max_blocks);
/* fp32 NT kernel: 1 (default) four dedicated loader waves per block issue the LDS-DMA, 0 the four compute waves stage
 * their own operands (A/B; same results). */
int aew_set_nf_loaders(int on);
/* default NT shape only: 192 x 128 tiles (8 waves of 48x64) instead of 256 x 128 — 0 never, 1 (default) where the
 * per-CU cost model prefers them, 2 always.  Results are bit-identical either way. */
int aew_set_nt_rows192(int mode);
/* default NT shape only: descriptors whose first two segments are the SAME buffer at row offsets d <= max_dist apart
 * (the two taps of a dilated convolution, wavenet.py:100-101, and of its input gradient) stage ONE LDS window of
 * 256 + d rows per K tile and issue both taps' MFMAs from it (k_gemm_nt_bf16_win).  Default 64 (the largest
 * supported), 0 = never.  Results agree with the two-segment kernel to fp32 accumulation order, not bit for bit. */
int aew_set_nt_window(int max_dist);
/* 1 (default): STORE and DFG launches of the default 256- / 192-row bf16 NT bodies, of the one-window body and the
 * chained launches whose STORE / DFG stages all qualify store and load their epilogue rows as whole 128-byte lines: the
 * accumulators of a 16-row group are exchanged across lanes so that a wave access covers 8 rows x 128 B instead of
 * 16 rows x 64 B.  0: the MFMA-layout epilogue.  Bit-identical results; fp32 views, AEW_EF_COUNT_ZERO and every other
 * shape run the MFMA-layout epilogue under either value.  Read at LAUNCH time (a captured graph keeps the form it was
 * captured under); no plan, stage table or record depends on it.  Process-wide; not a field of aew_tuning_t. */
int aew_set_nt_epi_lines(int on);
/* 0 (default): ignore aew_op_t.lane - every op on the caller's stream, in plan order.  1: side-lane ops on private
 * streams (branches of a captured graph).  Same results either way (the atomically accumulated bias sums up to order). */
int aew_set_lanes(int on);
/* Row cursor of the grouped weight-gradient launch: a launch whose descriptor carries progress words
 * (aew_gemm_tn_group_t.cursors) is paced.  epoch = 32-row stages per epoch, slack = epochs a tile may run ahead of the slowest
 * tile of its matrix: (0, -) = the defaults 4 / 2 (the process default); (3..64, 1..8) explicit; (-1, -) = never pace. */
int aew_set_tn_cursor(int epoch, int slack);

/* Number of fp32 partial slabs a TN op writes into `out` (depends on the split heuristic). */
int aew_tn_slabs(const aew_gemm_tn_t* g);
/* ABI 26, test and measurement aid: what the TN launchers decide under the current settings, without launching.  Their return
 * code for a descriptor / group they refuse (*out untouched), else 0 and the row of the library's table of TN kernel instantiations
 * (name as written there; bk x bn its output tile), block, LDS, grid, the tile and rows per stage, the split-K plan | the cursor */
typedef struct { int32_t row, bk, bn, threads, lds_bytes, grid[3], tile, rc, splits, rows_per_split, fold, slabs, cursor, cursor_epoch, cursor_slack; char name[96]; } aew_tn_pick_t;
int aew_tn_pick(const aew_gemm_tn_t* g, aew_tn_pick_t* out);
int aew_tn_group_pick(const aew_gemm_tn_group_t* p, aew_tn_pick_t* out);
/* (k tiles, n tiles) of g's output under a group tile of 128 | 256 | 384: tile_map's tile = nt * *nkt + kt.  Host logic only. */
int aew_tn_group_tiles(const aew_gemm_tn_t* g, int tile, int* nkt, int* nnt);
/* Validate one descriptor of a grouped launch (aew_gemm_tn_group_t.descs lives in device memory, so the launcher
 * cannot): 0 or AEW_E_*.  Host logic only. */
int aew_tn_group_check(const aew_gemm_tn_t* g);
/* What the deterministic form of a column-sum op needs (aew_colsum_t.det_scratch / det_tickets): *floats of scratch,
 * *tickets words (zeroed once by the caller).  Host logic only; the launcher uses the same arithmetic. */
int aew_colsum_det_size(const aew_colsum_t* c, int64_t* floats, int32_t* tickets);
/* 1 if the op's batch loop is folded into one slab per split (short contractions). */
int aew_tn_fold(const aew_gemm_tn_t* g);
/* Contraction length (rows x batch) up to which TN ops fold the batch; default 4096. */
int aew_set_tn_fold_rows(int rows);
/* Split-K target of the TN ops (blocks per launch, default 512).  Changes aew_tn_slabs(): set it
 * before building a plan. */
int aew_set_tn_target_blocks(int n);
/* TN ops whose output has <= max_tiles 128x128 tiles are split to ~target_blocks blocks only (fewer
 * slabs).  Like the call above it changes aew_tn_slabs(): set before building a plan. */
int aew_set_tn_small(int max_tiles, int target_blocks);
/* 1: read TN fragments with a scalar LDS gather instead of ds_read_b64_tr_b16 (debug aid). */
int aew_set_tn_safe(int on);
/* 256 x 256 output tiles for large bf16 wgrads (k_gemm_tn_bf16_big): on = 0 / 1, target_blocks > 0 sets the split-K
 * block target.  Changes the slab count: call before plans are built (aew_tn_slabs follows it). */
int aew_set_tn_big(int on, int target_blocks);

/* =======================================================================================
 * Autoregressive sampler — replaces WaveNet.forward_test (wavenet.py:367-531: the per-sample Python
 * loop over base_layer / conv_layers / post1 / post2 / softmax / torch.multinomial with rolling
 * per-layer buffers, driven by InferenceChassis, chassis.py:283-349).
 *
 * One PERSISTENT kernel; every wavefront is an ACTOR that owns a fixed slice of one layer's weights
 * (MFMA A-fragments resident in its VGPRs for the whole generation) and processes the work items
 * (t, b) — time step t of stream-batch b, 16 streams per batch — in the same global order
 * t = 0..n_steps-1, b = 0..n_batches-1.  Actors exchange 16-stream activation rows through global
 * memory and signal with monotone sequence flags: flag = seq(t, b) = t*n_batches + b + 1 once item
 * (t, b) is published.  Per layer l (dilation d):
 *   EARLY(l,p)  pre-activations of channel pair-tile p from h_l(t-d) and cond(t)  (off the critical path)
 *   LATE(l,p)   adds the h_l(t) taps, gates: z_l = tanh(filt)*sigmoid(gate)          (wavenet.py:100-103)
 *   RES(l,q)    h_{l+1}(t) = h_l(t) + W_res z_l                                      (wavenet.py:108-110)
 *   SKIP(l,q)   skip sum += W_skp z_l                                                (wavenet.py:104,458)
 * then POST1 / POST2 (wavenet.py:461-462) and SAMPLE (softmax + inverse-CDF draw from a counter RNG in
 * place of torch.multinomial, wavenet.py:463-466; writes the base-layer row h_0(t+1), wavenet.py:452).
 * With n_batches > 1 the layers work on different stream-batches at the same time (a pipeline).
 * Every spin is bounded: if a producer never arrives the kernel sets status[0] and all actors exit.
 * ===================================================================================== */
#define AEW_ACT_NONE   (-1)
#define AEW_ACT_EARLY  0
#define AEW_ACT_LATE   1
#define AEW_ACT_RES    2
#define AEW_ACT_SKIP   3
#define AEW_ACT_POST1  4
#define AEW_ACT_POST2  5
#define AEW_ACT_SAMPLE 6

/* 16-stream activation buffer.  Entry of stream-batch b at time t (BYTES): ptr + b*bstride + (t % ring)*entry.
 * layout 0 (rows): stream i's channels are contiguous, row at + i*pitch.
 * Rows that several actors write are stored PRODUCER-CONTIGUOUS instead, so that every actor writes whole cache
 * lines of its own and a consumer's K tile (32 channels x 16 streams) is one 1 KiB block:
 * layout 1 (h_l, relu(post1)): [32-channel group][stream][32 ch]  -> channel c of stream i at (c/32)*1024 + i*64 + (c%32)*2
 * layout 2 (z_l):              [16-channel pair ][stream][16 ch]  -> (c/16)*512 + i*32 + (c%16)*2 */
typedef struct {
    void*   ptr;
    int64_t bstride;
    int64_t entry;
    int64_t pitch;
    int32_t ring;                /* >= 1 */
    int32_t layout;
} aew_sbuf_t;

/* wait until flags[j*flag_stride] >= seq(t - lag, b) for j < n (skipped while t < lag) */
typedef struct {
    const uint32_t* flags;
    int32_t n;                   /* <= 32 */
    int32_t lag;
} aew_wait_t;

typedef struct {
    int32_t role;                /* AEW_ACT_* */
    int32_t layer, index;        /* informational */
    int32_t nt;                  /* 16-channel output tiles this actor owns: 1 or 2                       */
    int32_t nk;                  /* K tiles (32 channels) of the register-resident weights `w`             */
    int32_t nk2;                 /* EARLY: K tiles of the streamed cond weights `w2`                       */
    int32_t dil;                 /* EARLY: dilation d                                                      */
    int32_t pad;
    aew_wait_t wait[2];
    uint32_t* flag;              /* this actor's sequence flag                                             */
    /* weight fragments, bf16: blob[k][n(2)][lane(64)][8] = W[n*16 + (lane&15)][k*32 + (lane>>4)*8 + j]
     * (the MFMA 16x16x32 A operand); SAMPLE: `w` = base-layer table [Q][in0-row] bf16 (bias folded in)  */
    const void* w;
    const void* w2;
    /* fp32 bias: EARLY per stream [n_streams][bias_pitch] (speaker term folded in), lane reads
     * bias[stream*bias_pitch + n*16 + (lane>>4)*4 .. +3]; POST1/POST2 shared (bias_pitch = 0)            */
    const float* bias;
    int64_t bias_pitch;
    /* role        in0                  in1                      out
     * EARLY       h_l (read at t-d)    cond (ring = n_steps)    partial pre-acts (ring 2; raw lane layout)
     * LATE        h_l (t)              partial pre-acts         z_l     (ptr at this pair's channels)
     * RES         z_l                  h_l (t), own channels    h_{l+1} (t), own channels
     * SKIP        z_l                  skip sum (NULL: layer 0) skip sum, own channels (fp32)
     * POST1       skip sum (fp32)      -                        relu(post1) bf16, own channels
     * POST2       relu(post1)          -                        logits fp32, own channels
     * SAMPLE      logits               -                        h_0 (written at t+1)                        */
    aew_sbuf_t in0, in1, out;
    aew_sbuf_t out2;             /* POST2: optional copy of the logits (ring = n_steps), ptr NULL = off     */
    int32_t n_quant;             /* SAMPLE: Q (multiple of 16, <= 256); streams [index*4, index*4+4)        */
    int32_t row_bytes;           /* SAMPLE: bytes of one base-table row (= h_0 row)                         */
} aew_actor_t;

/* Draw controls of ONE stream (appended to ABI 28; aew_sizeof 41 - index 40 stays unused, it answers -1): sampling
 * temperature, top-k, nucleus (top-p) and greedy, applied by the SAMPLE actor between the logits POST2 wrote and the value
 * it feeds.  THE RULE, for one stream at one step with fp32 logits l[0..Q) and the uniform u the draw already uses
 * (aew_jitter_u(seed, 0x53414d50, stream, t + 1): the same number with controls on or off):
 *   order    value i precedes value j when l[i] > l[j], or l[i] == l[j] and i < j (a total order, ties to the lower index)
 *   greedy   (flags & 1): the value fed is the first in the order; u is not used
 *   weights  w[i] = exp((l[i] - max l) * inv_temp) in fp32 (__expf of the fp32 product); inv_temp == 1.0f: today's weights
 *   K-set    the first top_k values in the order; top_k <= 0 or top_k >= Q: all of them
 *   P-set    the shortest prefix of the K-set, in the order, whose weight sum is at least top_p times the K-set's; never
 *            empty; top_p >= 1: the whole K-set; top_p <= 0: exactly the first value
 *   draw     weights outside the P-set are zero, then the draw of aew_sampler_run as it was: sums in index order (per lane
 *            over its Q / 16 values, inclusive scan over the stream's 16 lanes), the drawn value is the first index whose
 *            running sum exceeds u * total, or the last kept index if rounding leaves none.
 * (1.0, 0, 1.0, 0) is neutral: the draw without controls, bit for bit.  Forced positions stay forced.  Whatever a record
 * holds, the value fed lies in [0, Q). */
typedef struct {
    float   inv_temp;            /* 1 / temperature                                                         */
    int32_t top_k;               /* <= 0 or >= Q: off                                                       */
    float   top_p;               /* >= 1: off; <= 0: the first value alone                                  */
    int32_t flags;               /* bit 0: greedy                                                           */
} aew_draw_t;

typedef struct {
    const aew_actor_t* actors;   /* DEVICE array [n_slots]; slot L runs as workgroup L (XCD L % 8)          */
    int32_t n_slots;
    int32_t n_batches;           /* stream-batches of 16 streams                                          */
    int32_t n_steps;             /* T: positions 0..T-1; position 0 is always forced                       */
    int32_t flag_stride;         /* uint32 words between consecutive flags                                 */
    int32_t kr_max;              /* 12 or 16: compiled bound on nk of EARLY / LATE                         */
    int32_t spin_max;            /* polls before an actor gives up (0 = default)                           */
    uint32_t* flags;             /* [n_slots * flag_stride]; zeroed by aew_sampler_run                      */
    uint32_t* status;            /* [4] device words: abort flag, slot, t, b of the first give-up          */
    const int32_t* forced;       /* [n_streams][n_steps]: value fed at position t if >= 0, else the draw   */
    int32_t* wav_out;            /* [n_streams][n_steps] the sequence that was fed (forced or drawn)       */
    uint64_t seed;               /* u(stream, t) = mix64-counter uniform, see oracle/jitter_rng.py         */
    int32_t nap_eighths;         /* 0..7: after publishing an item an actor sleeps through this many eighths of the
                                    running average of its own item period before it polls again (fewer pollers
                                    on the memory-side path); 0 = poll at once                                */
    int32_t pad;
    uint64_t* prof;              /* optional [n_slots][4]: s_memtime cycles (100 MHz) each actor spent waiting,
                                    loading + computing, publishing; [3] = items.  NULL = off               */
    const aew_draw_t* draw;      /* appended to ABI 28, optional DEVICE array [16 * n_batches], one record per stream,
                                    constant during the run.  NULL = the draw and the kernel of before, bit for bit;
                                    non-NULL launches the second instantiation of the kernel (same actors, same
                                    protocol), whose SAMPLE actors apply the records                         */
} aew_sampler_t;

/* Enqueue one generation on `stream`.  Returns AEW_E_UNSUP if the device cannot keep n_slots
 * wavefront-workgroups resident at once (the actors wait on each other). */
int aew_sampler_run(const aew_sampler_t* s, void* stream);

/* Human-readable string for a return code. */
const char* aew_strerror(int code);

/* Device self-test of the MFMA / LDS-transpose lane mappings this library relies on.
 * scratch: >= 1 MiB device buffer.  Returns 0 if the hardware behaves as assumed. */
int aew_selftest(void* scratch, int64_t scratch_bytes, void* stream, int32_t* detail /*[8]*/);

#ifdef __cplusplus
}
#endif
#endif /* AEWAVENET_H */
