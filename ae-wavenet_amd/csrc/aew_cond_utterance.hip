// aew_cond_utterance.hip — whole utterances through the fixed-geometry conditioning chain: AEW_OP_CODE_TILE fills the
// engine's code and voice inputs with windows cut out of a flat code buffer (code 0 where an utterance has none),
// AEW_OP_COND_STITCH moves the conditioning rows each window owns - and the gated bias of an utterance's first window - to
// their place in the per-stream buffers the sampler reads.  Both read one device-resident table of aew_cond_row_t
// (aewavenet.h states the contract).  Byte movers; the only atomic is the count of codes outside the codebook.
// Part of the library's one translation unit (aewavenet.hip includes it).
#pragma once
#include "aew_common.h"

// ---- the records' checks, ONE definition for the launchers (host copy of the table) and the kernels (device copy)
// codes of the window that are read - hi - lo, 0 for an idle row - or -1 for a record AEW_OP_CODE_TILE refuses: the reads
// of a good record stay inside [0, n_codes)
__host__ __device__ __forceinline__ int32_t cond_tile_n(const aew_cond_row_t& r, int E, int64_t n_codes, int n_voice) {
    return r.utt < 0 ? 0 : code_window_n(r, E, n_codes, n_voice);
}
// rows of the window that are moved, 0 for an idle row, or -1 for a record AEW_OP_COND_STITCH refuses: the reads of a good
// record stay inside the T rows of cond[b], its writes inside stream r.stream of cond_utt (n_dst elements) and of bias_utt
__host__ __device__ __forceinline__ int32_t cond_stitch_n(const aew_cond_row_t& r, int T, int Cp, int n_streams, int64_t n_dst) {
    if (r.utt < 0) return 0;
    if (r.n_rows < 0 || r.src_row < 0 || r.n_rows > T || r.src_row > T - r.n_rows) return -1;
    if (r.stream < 0 || r.stream >= n_streams || r.pitch < 1) return -1;
    if (r.dst_row < 0 || r.n_rows > r.pitch || r.dst_row > r.pitch - r.n_rows) return -1;
    const int64_t per = (int64_t)r.pitch * Cp;                                  // elements of one stream, < 2^62
    if (per > n_dst || (int64_t)r.stream > n_dst / per - 1) return -1;          // (stream + 1) * per <= n_dst
    return r.n_rows;
}

// ---- AEW_OP_CODE_TILE
// One wave per batch row.  The record is read through the kernel argument at a block-uniform index, so every lane holds
// the same values; a record that fails the launcher's check (the table changed under a captured graph) is treated as
// idle.  A code is tested against [0, K) before it is stored; each lane adds its own count of the ones that fail.
__global__ __launch_bounds__(AEW_WAVE) void k_code_tile(const aew_code_tile_t p) {
    const int b = blockIdx.x;
    const aew_cond_row_t r = p.table[(int64_t)p.first_row + b];
    const int32_t n = cond_tile_n(r, p.E, p.n_codes, p.n_voice);
    const bool live = r.utt >= 0 && n >= 0;
    const unsigned int bad = code_window_cut<AEW_WAVE>(p, r, live, b);
    if (bad) atomicAdd(p.bad, bad);
    if (threadIdx.x == 0) p.in_voice[b] = live ? (int64_t)r.voice : 0;
}

static int launch_code_tile(const aew_code_tile_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.codes || !p.ind || !p.in_voice || !p.bad || p.E < 1 || p.K < 1 || p.n_voice < 1 || p.n_codes < 0) return AEW_E_ARG;
    if (((uintptr_t)p.codes | (uintptr_t)p.ind | (uintptr_t)p.in_voice) & 15) return AEW_E_ALIGN;
    if ((uintptr_t)p.bad & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return cond_tile_n(r, p.E, p.n_codes, p.n_voice); })) return AEW_E_ARG;
    hipLaunchKernelGGL(k_code_tile, dim3((unsigned)p.B), dim3(AEW_WAVE), 0, st, p);
    return (int)hipGetLastError();
}

// ---- AEW_OP_COND_STITCH
#define AEW_CONDST_THREADS 256

// grid (x, B): the threads of batch row b walk the row's n_rows * Cp / 8 vectors of 16 bytes (8 bf16) with the stride of
// the whole x extent, then - for an utterance's first window - the bias_n / 4 vectors of its gated bias.  Source rows lie
// cond_pitch apart, destination rows Cp.  A record that fails the launcher's check stores nothing.
__global__ __launch_bounds__(AEW_CONDST_THREADS) void k_cond_stitch(const aew_cond_stitch_t p) {
    const int b = blockIdx.y;
    const aew_cond_row_t r = p.table[(int64_t)p.first_row + b];
    const int32_t n = cond_stitch_n(r, p.T, p.Cp, p.n_streams, p.n_dst);
    if (r.utt < 0 || n < 0) return;
    const int64_t step = (int64_t)gridDim.x * AEW_CONDST_THREADS;
    const int64_t q0 = (int64_t)blockIdx.x * AEW_CONDST_THREADS + threadIdx.x;
    const int vpr = p.Cp / 8;                                                   // vectors per row
    const uint16_t* src = p.cond + (int64_t)b * p.cond_bs + (int64_t)r.src_row * p.cond_pitch;
    uint16_t* dst = p.cond_utt + ((int64_t)r.stream * r.pitch + r.dst_row) * p.Cp;
    const int64_t n_vec = (int64_t)n * vpr;
    for (int64_t q = q0; q < n_vec; q += step) {
        const int64_t row = q / vpr;
        const int v = (int)(q - row * vpr);
        *reinterpret_cast<uint4*>(dst + row * p.Cp + 8 * v) = *reinterpret_cast<const uint4*>(src + row * p.cond_pitch + 8 * v);
    }
    if (r.first) {
        const float* bs = p.bias + (int64_t)b * p.bias_n;
        float* bd = p.bias_utt + (int64_t)r.stream * p.bias_n;
        for (int64_t q = q0; q < p.bias_n / 4; q += step)
            *reinterpret_cast<float4*>(bd + 4 * q) = *reinterpret_cast<const float4*>(bs + 4 * q);
    }
}

static int launch_cond_stitch(const aew_cond_stitch_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.cond || !p.cond_utt || !p.bias || !p.bias_utt || p.T < 1 || p.Cp < 8 || (p.Cp & 7) || p.cond_pitch < p.Cp ||
        (p.cond_pitch & 7) || p.cond_bs < 0 || (p.cond_bs & 7) || p.bias_n < 4 || (p.bias_n & 3) || p.n_streams < 1 || p.n_dst < 0)
        return AEW_E_ARG;
    if (((uintptr_t)p.cond | (uintptr_t)p.cond_utt | (uintptr_t)p.bias | (uintptr_t)p.bias_utt) & 15) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return cond_stitch_n(r, p.T, p.Cp, p.n_streams, p.n_dst); })) return AEW_E_ARG;
    const int64_t per_row = (int64_t)p.T * (p.Cp / 8);
    int64_t gx = (per_row + AEW_CONDST_THREADS - 1) / AEW_CONDST_THREADS;
    if (gx > 1024) gx = 1024;                                                   // (the loops stride over the rest)
    hipLaunchKernelGGL(k_cond_stitch, dim3((unsigned)gx, (unsigned)p.B), dim3(AEW_CONDST_THREADS), 0, st, p);
    return (int)hipGetLastError();
}
