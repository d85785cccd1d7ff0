// aew_score.hip — whole utterances through the teacher-forced decoder: AEW_OP_WAV_TILE fills the engine's waveform, code
// and voice inputs with windows cut out of the flat buffers (the zero-amplitude code / code 0 where an utterance has
// nothing), AEW_OP_NLL_STITCH moves the per-position NLL - and target probability, and top-1 hit - of the outputs each
// window owns to their place in the flat per-utterance arrays, AEW_OP_SCORE_REDUCE sums every utterance's range in the
// fixed order of aew_eval_acc_t.  The first two read one device-resident table of aew_score_row_t (aewavenet.h states the
// contract).  Plain loads and stores; the only atomics are the integer counts of values outside their range.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_ops.hip, whose eval_tree it uses).
#pragma once
#include "aew_common.h"

// ---- the records' checks, ONE definition for the launchers (host copy of the table) and the kernels (device copy)
// 1 for a live row AEW_OP_WAV_TILE serves, 0 for an idle one, -1 for a record it refuses: the reads of a good record stay
// inside [0, n_codes) and [0, n_wav)
__host__ __device__ __forceinline__ int32_t score_tile_n(const aew_score_row_t& r, int E, int64_t n_codes, int n_voice, int64_t n_wav) {
    if (r.utt < 0) return 0;
    if (code_window_n(r, E, n_codes, n_voice) < 0) return -1;
    if (r.wav_len < 0 || r.wav_base < 0 || r.wav_len > n_wav || r.wav_base > n_wav - r.wav_len) return -1;
    const int64_t lim = (int64_t)1 << 40;
    if (r.wav0 <= -lim || r.wav0 >= lim) return -1;
    return 1;
}
// outputs of the window that are moved, 0 for an idle row, or -1 for a record AEW_OP_NLL_STITCH refuses: the reads of a
// good record stay inside the positions [0, w - 1) of row b, its writes inside [0, n_dst)
__host__ __device__ __forceinline__ int32_t score_stitch_n(const aew_score_row_t& r, int w, int64_t n_dst) {
    if (r.utt < 0) return 0;
    if (r.n_out < 0 || r.src < 0 || r.n_out > w - 1 || r.src > w - 1 - r.n_out) return -1;
    if (r.dst < 0 || r.n_out > n_dst || r.dst > n_dst - r.n_out) return -1;
    return r.n_out;
}

// ---- AEW_OP_WAV_TILE
#define AEW_SCORE_THREADS 256

// grid (x, B): the threads of batch row b walk its T decoder-input samples with the stride of the whole x extent; block
// x = 0 also writes the row's E codes and its voice.  The record is read at a block-uniform index; one that fails the
// launcher's check (the table changed under a captured graph) is treated as idle.  A value is tested against its range
// before it is stored; each thread adds its own count of the ones that fail.
__global__ __launch_bounds__(AEW_SCORE_THREADS) void k_wav_tile(const aew_wav_tile_t p) {
    const int b = blockIdx.y;
    const aew_score_row_t r = p.table[(int64_t)p.first_row + b];
    const bool live = score_tile_n(r, p.E, p.n_codes, p.n_voice, p.n_wav) > 0;
    float* dst = p.wav + (int64_t)b * p.wav_pitch + p.wav_off;
    const float nq = (float)p.n_quant;
    unsigned int bad = 0;
    for (int t = blockIdx.x * AEW_SCORE_THREADS + threadIdx.x; t < p.T; t += gridDim.x * AEW_SCORE_THREADS) {
        float v = p.zero;
        const int64_t pos = r.wav0 + t;
        if (live && pos >= 0 && pos < r.wav_len) {
            v = p.wavs[r.wav_base + pos];
            if (!(v >= 0.f && v < nq)) { v = p.zero; ++bad; }                   // (a NaN fails both comparisons)
        }
        dst[t] = v;
    }
    if (bad) atomicAdd(p.bad_wav, bad);
    if (blockIdx.x != 0) return;
    bad = code_window_cut<AEW_SCORE_THREADS>(p, r, live, b);
    if (bad) atomicAdd(p.bad_codes, bad);
    if (threadIdx.x == 0) p.in_voice[b] = live ? (int64_t)r.voice : 0;
}

static int launch_wav_tile(const aew_wav_tile_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.codes || !p.wavs || !p.ind || !p.in_voice || !p.wav || !p.bad_codes || !p.bad_wav) return AEW_E_ARG;
    if (p.E < 1 || p.K < 1 || p.n_voice < 1 || p.n_quant < 1 || p.T < 1 || p.n_codes < 0 || p.n_wav < 0 || p.wav_off < 0 ||
        p.wav_pitch < 1 || p.T > p.wav_pitch || p.wav_off > p.wav_pitch - p.T || !(p.zero >= 0.f && p.zero < (float)p.n_quant))
        return AEW_E_ARG;
    if (((uintptr_t)p.codes | (uintptr_t)p.wavs | (uintptr_t)p.ind | (uintptr_t)p.in_voice | (uintptr_t)p.wav) & 15) return AEW_E_ALIGN;
    if (((uintptr_t)p.bad_codes | (uintptr_t)p.bad_wav) & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return score_tile_n(r, p.E, p.n_codes, p.n_voice, p.n_wav); })) return AEW_E_ARG;
    int gx = (p.T + AEW_SCORE_THREADS - 1) / AEW_SCORE_THREADS;
    if (gx > 64) gx = 64;                                                       // (the loop strides over the rest)
    hipLaunchKernelGGL(k_wav_tile, dim3((unsigned)gx, (unsigned)p.B), dim3(AEW_SCORE_THREADS), 0, st, p);
    return (int)hipGetLastError();
}

// ---- AEW_OP_NLL_STITCH
// grid (x, B): the threads of batch row b walk the row's n_out owned outputs.  A record that fails the launcher's check
// stores nothing.
__global__ __launch_bounds__(AEW_SCORE_THREADS) void k_nll_stitch(const aew_nll_stitch_t p) {
    const int b = blockIdx.y;
    const aew_score_row_t r = p.table[(int64_t)p.first_row + b];
    const int32_t n = score_stitch_n(r, p.w, p.n_dst);
    if (n <= 0) return;
    const int64_t row = (int64_t)b * p.w;
    for (int i = blockIdx.x * AEW_SCORE_THREADS + threadIdx.x; i < n; i += gridDim.x * AEW_SCORE_THREADS) {
        const int u = r.src + i;
        p.dst_nll[r.dst + i] = p.nll[row + u];
        if (p.dst_ptgt) p.dst_ptgt[r.dst + i] = p.ptgt[row + u];
        if (p.dst_hit) {
            const int tgt = (int)p.wav[(int64_t)b * p.wav_pitch + p.tgt_off + u + 1];
            int am = 0;
            if (p.amax) am = p.amax[row + u];
            else {
                // the fallback of engines whose softmax writes no arg-max: one thread scans its position's n_quant logits,
                // a pitch apart from its neighbour's.  Correct, covered at the op level only, and its rate is unmeasured -
                // the engines built today all write amax.
                const float* lg = p.logits + (int64_t)b * p.bs + (int64_t)u * p.pitch;
                float best = lg[0];
                for (int c = 1; c < p.n_quant; ++c) {
                    const float v = lg[c];
                    if (v > best) { best = v; am = c; }                         // strictly greater: the lowest class keeps a tie
                }
            }
            p.dst_hit[r.dst + i] = am == tgt ? (uint8_t)1 : (uint8_t)0;
        }
    }
}

static int launch_nll_stitch(const aew_nll_stitch_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.nll || !p.dst_nll || (p.dst_ptgt && !p.ptgt) || p.w < 2 || p.n_dst < 0) return AEW_E_ARG;
    if (p.dst_hit) {
        if (!p.wav || p.tgt_off < 0 || p.wav_pitch < 1 || p.w > p.wav_pitch || p.tgt_off > p.wav_pitch - p.w) return AEW_E_ARG;
        if (!p.amax && (!p.logits || p.n_quant < 1 || p.pitch < p.n_quant || p.bs < 0)) return AEW_E_ARG;
    }
    if (((uintptr_t)p.nll | (uintptr_t)p.ptgt | (uintptr_t)p.amax | (uintptr_t)p.logits | (uintptr_t)p.wav | (uintptr_t)p.dst_nll |
         (uintptr_t)p.dst_ptgt) & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return score_stitch_n(r, p.w, p.n_dst); })) return AEW_E_ARG;
    int gx = (p.w + AEW_SCORE_THREADS - 1) / AEW_SCORE_THREADS;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(k_nll_stitch, dim3((unsigned)gx, (unsigned)p.B), dim3(AEW_SCORE_THREADS), 0, st, p);
    return (int)hipGetLastError();
}

// ---- AEW_OP_SCORE_REDUCE
// One block of 1024 threads per utterance.  Thread t adds its elements t, t + 1024, ... ascending in double, then the
// halving tree of the evaluation accumulator (eval_tree, aew_ops.hip) - separately for the three sums.
__global__ __launch_bounds__(1024) void k_score_reduce(const aew_score_reduce_t p) {
    __shared__ double sh[1024];
    const int u = blockIdx.x, t = threadIdx.x;
    int64_t lo = p.offsets[u], hi = p.offsets[u + 1];
    if (lo < 0 || hi < lo || hi > p.n_src) lo = hi = 0;                          // (the table changed under a captured graph)
    const int64_t n = hi - lo;
    double s_nll = 0.0, s_pt = 0.0, s_hit = 0.0;
    for (int64_t i = lo + t; i < hi; i += 1024) {
        s_nll += (double)p.nll[i];
        if (p.ptgt) s_pt += (double)p.ptgt[i];
        if (p.hit) s_hit += p.hit[i] ? 1.0 : 0.0;
    }
    const double b_nll = eval_tree(sh, s_nll), b_pt = eval_tree(sh, s_pt), b_hit = eval_tree(sh, s_hit);
    if (t != 0) return;
    double* acc = p.acc + 4 * (int64_t)u;
    float* out = p.out + 4 * (int64_t)u;
    acc[0] = (double)n; acc[1] = b_nll; acc[2] = b_pt; acc[3] = b_hit;
    auto div = [](double x, double y) { return y > 0.0 ? x / y : 0.0; };
    const double nll = div(b_nll, (double)n);
    out[0] = (float)nll;
    out[1] = (float)(nll / 0.693147180559945309417232121458);
    out[2] = (float)div(b_hit, (double)n);
    out[3] = (float)div(b_pt, (double)n);
}

static int launch_score_reduce(const aew_score_reduce_t& p, hipStream_t st) {
    if (!p.offsets || !p.offsets_host || !p.nll || !p.acc || !p.out || p.U < 1 || p.U > (1 << 20) || p.n_src < 0) return AEW_E_ARG;
    if (((uintptr_t)p.offsets | (uintptr_t)p.offsets_host | (uintptr_t)p.acc) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.nll | (uintptr_t)p.ptgt | (uintptr_t)p.out) & 3) return AEW_E_ALIGN;
    if (p.offsets_host[0] < 0 || p.offsets_host[p.U] > p.n_src) return AEW_E_ARG;
    for (int u = 0; u < p.U; ++u)
        if (p.offsets_host[u + 1] < p.offsets_host[u]) return AEW_E_ARG;
    hipLaunchKernelGGL(k_score_reduce, dim3((unsigned)p.U), dim3(1024), 0, st, p);
    return (int)hipGetLastError();
}
