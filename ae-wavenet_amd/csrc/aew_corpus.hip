// aew_corpus.hip — the device-resident training corpus: AEW_OP_WINDOW_GATHER cuts a batch's windows out of a corpus held
// in device memory (aew_window_gather_t in aewavenet.h states the contract; the reference: data.py SliceDataset.__getitem__,
// LoopingRandomSampler.__iter__, TrackerDataset.__getitem__, Collate.__call__ line 229).  Part of the library's one
// translation unit (aewavenet.hip includes it).
#pragma once
#include "aew_common.h"

// ---- the index arithmetic, ONE definition for the kernel and for aew_corpus_locate (the CPU tests run this very code)
struct CorpusLoc {
    uint64_t epoch;              // sampler epoch e of item b (row e & 1 of `order`)
    int32_t p;                   // place in that epoch's permutation
    int64_t pos_epoch, pos_step; // TrackerDataset's (epoch, step) after the LAST item of the batch
};

__host__ __device__ __forceinline__ CorpusLoc corpus_locate(uint64_t t0, int b, int B, int64_t N, int n_order, int R) {
    CorpusLoc o;
    const uint64_t j = t0 + (uint64_t)b;
    o.epoch = j / (uint64_t)n_order;
    o.p = (int32_t)(j % (uint64_t)n_order);
    const uint64_t P = (uint64_t)((N + R - 1) / R), t = t0 + (uint64_t)B;
    o.pos_epoch = (int64_t)(t / P);
    o.pos_step = (int64_t)(t % P) * R;
    return o;
}

extern "C" int aew_corpus_locate(uint64_t t0, int b, int B, int64_t N, int n_order, int R, int rank, int* epoch, int* p,
                                 int64_t* pos_epoch, int64_t* pos_step) {
    if (!epoch || !p || !pos_epoch || !pos_step || B < 1 || b < 0 || b >= B || N < 1 || n_order < 1 || R < 1 || rank < 0 ||
        rank >= R)
        return AEW_E_ARG;
    const CorpusLoc o = corpus_locate(t0, b, B, N, n_order, R);
    if (o.epoch > 0x7fffffffull) return AEW_E_ARG;
    *epoch = (int)o.epoch; *p = o.p; *pos_epoch = o.pos_epoch; *pos_step = o.pos_step;
    return 0;
}

// ---- the kernel
#define AEW_WG_THREADS 256
#define AEW_WG_BLOCK_BYTES (AEW_WG_THREADS * 16)         // source bytes per block: one 16-byte piece per lane

// The 16 source bytes that start m bytes (0..15) into the aligned pair (lo, hi): two select stages move whole dwords, the
// byte-align instruction does the rest.  Branch-free, and every dword of both loads has a use, so the loads stay the
// two aligned 16-byte loads they are written as.
__device__ __forceinline__ void wg_realign(const uint4& lo, const uint4& hi, unsigned m, unsigned (&o)[4]) {
    unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const bool d2 = (m & 8) != 0, d1 = (m & 4) != 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = d2 ? w[k + 2] : w[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = d1 ? w[k + 1] : w[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], m & 3);       // ({hi, lo} >> 8 (m & 3))[31:0]
}

template <int BYTES> __device__ __forceinline__ float wg_elem(const void* snd, int64_t i);
template <> __device__ __forceinline__ float wg_elem<1>(const void* snd, int64_t i) { return (float)((const uint8_t*)snd)[i]; }
template <> __device__ __forceinline__ float wg_elem<2>(const void* snd, int64_t i) { return (float)((const int16_t*)snd)[i]; }
template <> __device__ __forceinline__ float wg_elem<4>(const void* snd, int64_t i) { return (float)((const int32_t*)snd)[i]; }

template <int BYTES>
__global__ __launch_bounds__(AEW_WG_THREADS) void k_window_gather(const aew_window_gather_t g) {
    constexpr int E = 16 / BYTES;                        // elements of one 16-byte piece
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint64_t t0 = *g.counter;                      // (the advance is a LATER launch: every block reads the same value)
    const CorpusLoc loc = corpus_locate(t0, b, g.B, g.N, g.n_order, g.num_replicas);
    const int32_t ord = g.order[(int64_t)(loc.epoch & 1) * g.n_order + loc.p];
    int64_t i = (int64_t)g.rank + (int64_t)g.num_replicas * ord;
    bool ok = ord >= 0 && ord < g.n_order && i < g.N;
    int64_t s = 0;
    if (ok) {
        s = g.starts[i];
        ok = s >= 0 && s <= g.n_snd - g.slice_size;
    }
    if (blockIdx.x == 0 && tid == 0) {
        g.voice[b] = ok ? (int64_t)g.voices[i] : -1;
        g.index[b] = ok ? (int32_t)i : -1;
        if (b == 0) { g.position[0] = loc.pos_epoch; g.position[1] = loc.pos_step; }
    }
    float* row = g.wav + (int64_t)b * g.wav_pitch;
    const int n_full = g.slice_size / E;                 // whole 16-byte pieces of the slice
    const int c = blockIdx.x * AEW_WG_THREADS + tid;     // this lane's piece: elements [c E, c E + E) of the slice
    if (c < n_full) {
        unsigned o[4] = {0u, 0u, 0u, 0u};
        if (ok) {
            // bytes [a, a + 16) of the corpus, a >= 0 and a + 16 <= BYTES * n_snd: the aligned quantity that holds byte a
            // starts at or above snd, the next one starts below the corpus' end and so ends inside the 16 bytes of slack
            const int64_t a = (s + (int64_t)c * E) * BYTES;
            const uint4* q = (const uint4*)g.snd + (a >> 4);
            const uint4 lo = q[0], hi = q[1];
            wg_realign(lo, hi, (unsigned)(a & 15), o);
        }
        float4* dst = (float4*)(row + (int64_t)c * E);   // wav 16-byte aligned, wav_pitch % 4 == 0, E % 4 == 0
        if constexpr (BYTES == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                dst[k] = make_float4((float)(o[k] & 0xffu), (float)((o[k] >> 8) & 0xffu), (float)((o[k] >> 16) & 0xffu),
                                     (float)(o[k] >> 24));
        } else if constexpr (BYTES == 2) {
            dst[0] = make_float4((float)(int16_t)(o[0] & 0xffffu), (float)(int16_t)(o[0] >> 16),
                                 (float)(int16_t)(o[1] & 0xffffu), (float)(int16_t)(o[1] >> 16));
            dst[1] = make_float4((float)(int16_t)(o[2] & 0xffffu), (float)(int16_t)(o[2] >> 16),
                                 (float)(int16_t)(o[3] & 0xffffu), (float)(int16_t)(o[3] >> 16));
        } else {
            dst[0] = make_float4((float)(int32_t)o[0], (float)(int32_t)o[1], (float)(int32_t)o[2], (float)(int32_t)o[3]);
        }
    }
    // the slice_size % E elements behind the last whole piece, one by one (exact reads: no slack needed)
    const int tail = g.slice_size - n_full * E;
    if (blockIdx.x == gridDim.x - 1 && tid < tail) {
        const int k = n_full * E + tid;
        row[k] = ok ? wg_elem<BYTES>(g.snd, s + k) : 0.f;
    }
}

__global__ void k_window_advance(uint64_t* counter, uint64_t n) { *counter += n; }

static int window_gather_check(const aew_window_gather_t& g) {
    if (g.B < 1 || g.slice_size <= 0 || (g.snd_bytes != 1 && g.snd_bytes != 2 && g.snd_bytes != 4)) return AEW_E_ARG;
    if (g.num_replicas < 1 || g.rank < 0 || g.rank >= g.num_replicas || g.N < 1 || g.n_order < g.B) return AEW_E_ARG;
    if (g.rank >= g.N || (int64_t)g.n_order != (g.N - g.rank + g.num_replicas - 1) / g.num_replicas) return AEW_E_ARG;
    if (g.n_snd < g.slice_size || g.wav_pitch < g.slice_size || (g.wav_pitch & 3) || g.B > 65535) return AEW_E_ARG;
    if (!g.snd || !g.starts || !g.voices || !g.order || !g.counter || !g.wav || !g.voice || !g.index || !g.position)
        return AEW_E_ARG;
    if (((uintptr_t)g.snd | (uintptr_t)g.wav) & 15) return AEW_E_ALIGN;
    if (((uintptr_t)g.starts | (uintptr_t)g.counter | (uintptr_t)g.voice | (uintptr_t)g.position) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)g.voices | (uintptr_t)g.order | (uintptr_t)g.index) & 3) return AEW_E_ALIGN;
    return 0;
}

static int launch_window_gather(const aew_window_gather_t& g, hipStream_t st) {
    const int rc = window_gather_check(g);
    if (rc) return rc;
    const dim3 grid((unsigned)(((int64_t)g.slice_size * g.snd_bytes + AEW_WG_BLOCK_BYTES - 1) / AEW_WG_BLOCK_BYTES), (unsigned)g.B);
    if (g.snd_bytes == 1) hipLaunchKernelGGL(k_window_gather<1>, grid, dim3(AEW_WG_THREADS), 0, st, g);
    else if (g.snd_bytes == 2) hipLaunchKernelGGL(k_window_gather<2>, grid, dim3(AEW_WG_THREADS), 0, st, g);
    else hipLaunchKernelGGL(k_window_gather<4>, grid, dim3(AEW_WG_THREADS), 0, st, g);
    // stream order puts this behind every block's read of the counter
    if (g.advance) hipLaunchKernelGGL(k_window_advance, dim3(1), dim3(1), 0, st, g.counter, (uint64_t)g.B);
    return (int)hipGetLastError();
}
