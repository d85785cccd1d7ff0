// aew_segment.hip — AEW_OP_CODE_SEGMENT: the code sequence of whole utterances chosen jointly, a Viterbi pass over the K
// codebook entries with a uniform switch penalty (aewavenet.h states the rule bit for bit and the records' checks).
//
// Shape.  Two kernels of one op launch, ordered by the stream alone.
//   k_seg_cost   the hot one: the [n_rows][K] fp32 local costs into the workspace, parallel over (slab of SEG_SLAB frames
//                x group of 256 entries).  A lane owns ONE entry: for d <= 64 its row sits in registers for the whole slab
//                (DR floats, zeros behind d: u = 0 - 0, fma(0, 0, dd) = dd, the same bits) with sqrt(qq).  The frame is
//                wave-uniform: its d values come through the scalar path (a uniform address, a buffer the kernel never
//                writes), so the inner loop is a v_sub and a v_fma per channel and touches no vector memory; the frame's
//                norm was taken once per slab - lane l of every wave holds that of frame l and hands it over by a
//                uniform-index lane read.  One coalesced 256-byte store per wave and frame.  No LDS.
//   k_seg_scan   one WAVEFRONT per utterance: lane l keeps r for the entries l, l + 64, ... in registers (W = ceil(K / 64)
//                of them, the template steps 1, 2, 4 .. 64), reads cost row t coalesced with row t + 1 in flight, takes
//                (m, a) by a shuffle min-reduction under the rule's tie order, writes stay(t, .) as W ballot words and
//                A(t-1) into the utterance's back range; after the last frame lane 0 walks back, then all lanes fetch the
//                distances of the chosen codes.  It waits for no other wave: no flag, no spin, no barrier.
// The local cost, the recurrence step, the order of the minimum, the walk back and the records' checks are ONE
// __host__ __device__ definition each; aew_segment_host runs them on the CPU (fmaf in place of __fmaf_rn).
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_align.hip).
#pragma once
#include "aew_common.h"
#include <math.h>
#include <algorithm>
#include <utility>
#include <vector>

#define SEG_SLAB 64                // frames a block of k_seg_cost meets with its 256 entries: one norm per lane
#define SEG_GROUP 256              // entries per block of k_seg_cost

// ---- the arithmetic, ONE definition for the kernels and the host twin ----------------------------------------------------
__host__ __device__ __forceinline__ float seg_fma(float a, float b, float c) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fmaf_rn(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}
__host__ __device__ __forceinline__ float seg_sub(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
// one channel of the two chains of an (frame, entry) pair
__host__ __device__ __forceinline__ float seg_dd(float z, float e, float dd) {
    const float u = seg_sub(z, e);
    return seg_fma(u, u, dd);
}
// c(t, k) from the finished chains: zn = sqrt(zz) of the frame, sq = sqrt(qq) of the entry
__host__ __device__ __forceinline__ float seg_cost_of(float dd, float zn, float sq, int metric) {
#ifdef __HIP_DEVICE_COMPILE__
    return metric == 0 ? __fdiv_rn(sqrtf(dd), __fadd_rn(zn, sq)) : dd;
#else
    return metric == 0 ? sqrtf(dd) / (zn + sq) : dd;
#endif
}
// does (v, i) beat (best, bi)?  Strict '<' in ascending index order: the lowest index among ties, a NaN never wins
__host__ __device__ __forceinline__ bool seg_beats(float v, int i, float best, int bi) {
    return v < best || (v == best && i < bi);
}
// r(t, k) from r(t-1, k), the step's minimum, the penalty and c(t, k); *stay = stay(t, k)
__host__ __device__ __forceinline__ float seg_step(float rprev, float m, float lam, float c, bool* stay) {
    const float p = rprev - m;
    *stay = p < lam;
    return c + (*stay ? p : lam);
}
__host__ __device__ __forceinline__ int seg_words(int K) { return (K + 63) >> 6; }
__host__ __device__ __forceinline__ int64_t seg_cost_bytes(int64_t n_rows, int K) { return (n_rows * K * 4 + 7) & ~(int64_t)7; }
__host__ __device__ __forceinline__ int64_t seg_rows(int64_t n_elems, int d, int d_pitch) {
    return n_elems < d ? 0 : (n_elems - d) / d_pitch + 1;
}
// 1 if the utterance's rows lie inside [0, n_rows) and its back words inside the back region of n_rows * (W + 1) words
__host__ __device__ __forceinline__ int seg_rec_ok(const aew_seg_utt_t& r, int64_t n_rows, int K) {
    if (r.n_frames < 0 || !(r.lam >= 0.f)) return 0;
    if (r.n_frames == 0) return 1;
    if (r.first_frame < 0 || r.n_frames > n_rows || r.first_frame > n_rows - r.n_frames) return 0;
    const int64_t per = seg_words(K) + 1, need = (int64_t)r.n_frames * per, have = n_rows * per;
    return r.back_base >= 0 && need <= have && r.back_base <= have - need;
}
// the walk back over the back range of one utterance (rows of W + 1 words: stay bits, then A(t-1)); returns n_seg
__host__ __device__ __forceinline__ int seg_walk(const uint64_t* back, int W, int T, int K, int k, int64_t* codes) {
    int n_seg = 1;
    for (int t = T - 1; t >= 1; --t) {
        codes[t] = k;
        const uint64_t* row = back + (int64_t)t * (W + 1);
        if (!((row[k >> 6] >> (k & 63)) & 1)) {
            int a = (int)row[W];
            if ((unsigned)a >= (unsigned)K) a = 0;                               // (words that are no pass: stay inside the codebook)
            if (a != k) ++n_seg;
            k = a;
        }
    }
    codes[0] = k;
    return n_seg;
}

extern "C" int aew_segment_ws_bytes(int64_t n_rows, int K, int64_t* bytes) {
    if (!bytes || n_rows < 0 || K < 1 || K > AEW_SEG_MAX_K || n_rows > ((int64_t)1 << 40)) return AEW_E_ARG;
    *bytes = seg_cost_bytes(n_rows, K) + 8 * n_rows * (seg_words(K) + 1);
    return 0;
}

// ---- the checks of a call, ONE definition for the launcher and the host twin ---------------------------------------------
static int seg_check(const aew_code_segment_t& p, bool host, int64_t* n_rows_out) {
    if (!p.emb || !p.table_host || (!host && !p.table) || !p.codes || !p.cost || !p.n_seg || !p.n_bad || !p.ws) return AEW_E_ARG;
    if (p.metric != 0 && p.metric != 1) return AEW_E_ARG;
    if (p.K < 1 || p.K > AEW_SEG_MAX_K || p.d < 1 || p.d > AEW_SEG_MAX_D || p.d_pitch < p.d) return AEW_E_ARG;
    if (p.U < 0 || p.U > (1 << 24) || p.n_elems < 0 || p.n_elems > ((int64_t)1 << 50) || (p.n_elems > 0 && !p.frames)) return AEW_E_ARG;
    const int64_t n_rows = seg_rows(p.n_elems, p.d, p.d_pitch);
    if (n_rows > ((int64_t)1 << 40) || p.n_out < n_rows) return AEW_E_ARG;
    int64_t need = 0;
    if (aew_segment_ws_bytes(n_rows, p.K, &need) || p.ws_bytes < need) return AEW_E_ARG;
    if (((uintptr_t)p.table | (uintptr_t)p.table_host | (uintptr_t)p.codes | (uintptr_t)p.ws) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.frames | (uintptr_t)p.emb | (uintptr_t)p.dist | (uintptr_t)p.cost | (uintptr_t)p.n_seg | (uintptr_t)p.n_bad) & 3)
        return AEW_E_ALIGN;
    const int64_t per = seg_words(p.K) + 1;
    std::vector<std::pair<int64_t, int64_t>> held;                               // back ranges [lo, hi) of the utterances that own one
    for (int u = 0; u < p.U; ++u) {
        const aew_seg_utt_t& r = p.table_host[u];
        if (!seg_rec_ok(r, n_rows, p.K)) return AEW_E_ARG;
        if (r.n_frames > 0) held.emplace_back(r.back_base, r.back_base + r.n_frames * per);
    }
    std::sort(held.begin(), held.end());
    for (size_t i = 1; i < held.size(); ++i)
        if (held[i].first < held[i - 1].second) return AEW_E_ARG;
    *n_rows_out = n_rows;
    return 0;
}

// ---- k_seg_cost ----------------------------------------------------------------------------------------------------------
// DR > 0: d <= DR, the lane's entry in DR registers.  FULL: d == DR, the frame's channels are read as they stand (whole
// 64-byte scalar loads); otherwise channel j >= d is a zero, taken by a select behind a load at a clamped - in-bounds -
// index.  DR == 0: any d, the entry's row is read again for every frame.
template <int DR, bool FULL>
__global__ __launch_bounds__(SEG_GROUP) void k_seg_cost(const float* __restrict__ frames, const float* __restrict__ emb,
                                                        float* __restrict__ cost, const int64_t n_rows, const int K,
                                                        const int d, const int d_pitch, const int metric) {
    const int k = blockIdx.y * SEG_GROUP + threadIdx.x;
    const bool live = k < K;
    const int lane = threadIdx.x & 63;
    const int64_t f0 = (int64_t)blockIdx.x * SEG_SLAB;
    const int nf = n_rows - f0 < SEG_SLAB ? (int)(n_rows - f0) : SEG_SLAB;       // >= 1 (launcher)
    const float* erow = emb + (int64_t)(live ? k : K - 1) * d;                   // (idle lanes repeat the last entry: reads stay inside)
    float e[DR > 0 ? DR : 1];
    float qq = 0.f;
    if constexpr (DR > 0) {
#pragma unroll
        for (int j = 0; j < DR; ++j) e[j] = FULL ? erow[j] : (j < d ? erow[j] : 0.f);
#pragma unroll
        for (int j = 0; j < DR; ++j) qq = seg_fma(e[j], e[j], qq);
    } else {
        for (int j = 0; j < d; ++j) qq = seg_fma(erow[j], erow[j], qq);
    }
    const float sq = sqrtf(qq);                                                  // (IEEE-rounded, as in vq_scan)
    float zn_l = 0.f;                                                            // lane l: the norm of frame f0 + l
    if (metric == 0) {
        const float* zl = frames + (f0 + (lane < nf ? lane : nf - 1)) * d_pitch;
        float zz = 0.f;
        for (int j = 0; j < d; ++j) zz = seg_fma(zl[j], zl[j], zz);
        zn_l = sqrtf(zz);
    }
    float* out = cost + f0 * K + k;
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
        const float* z = frames + (f0 + f) * d_pitch;                            // wave-uniform
        float dd = 0.f;
        if constexpr (DR > 0) {
#pragma unroll
            for (int j = 0; j < DR; ++j) {
                float zj;
                if constexpr (FULL) zj = z[j];
                else { zj = z[j < d ? j : 0]; zj = j < d ? zj : 0.f; }
                dd = seg_dd(zj, e[j], dd);
            }
        } else {
            for (int j = 0; j < d; ++j) dd = seg_dd(z[j], erow[j], dd);
        }
        const float zn = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, zn_l), f));
        const float v = seg_cost_of(dd, zn, sq, metric);
        if (live) out[(int64_t)f * K] = v;
    }
}

// ---- k_seg_scan ----------------------------------------------------------------------------------------------------------
// (m, a) of the wave's W * 64 values r[i] of entry i * 64 + lane, in every lane; a = 0 where nothing is below +inf
template <int W>
__device__ __forceinline__ void seg_wave_min(const float (&r)[W], int lane, float& m, int& a) {
    float best = INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < W; ++i)
        if (r[i] < best) { best = r[i]; bi = i * 64 + lane; }                    // ascending k within the lane: the first minimum wins
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (seg_beats(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    m = best;
    a = bi == 0x7fffffff ? 0 : bi;
}

template <int W>
__global__ __launch_bounds__(64) void k_seg_scan(const aew_code_segment_t p, const int64_t n_rows) {
    const int u = blockIdx.x, lane = threadIdx.x;
    const aew_seg_utt_t rec = p.table[u];
    if (!seg_rec_ok(rec, n_rows, p.K)) return;                                   // wave-uniform, like every return below
    const int T = rec.n_frames, K = p.K, Wk = seg_words(K);
    if (T == 0) {
        if (lane == 0) { p.cost[u] = 0.f; p.n_seg[u] = 0; }
        return;
    }
    const float* cost = (const float*)p.ws + rec.first_frame * K;
    uint64_t* back = (uint64_t*)((char*)p.ws + seg_cost_bytes(n_rows, K)) + rec.back_base;
    const float lam = rec.lam;
    float r[W], cn[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int k = i * 64 + lane;
        r[i] = k < K ? cost[k] : INFINITY;                                       // (an entry that is none never wins and never stays)
        cn[i] = (T > 1 && k < K) ? cost[(int64_t)K + k] : INFINITY;
    }
    float acc = 0.f, m;
    int a;
    for (int t = 1; t < T; ++t) {
        float c[W];
#pragma unroll
        for (int i = 0; i < W; ++i) c[i] = cn[i];
        if (t + 1 < T) {                                                         // row t + 1, fetched under this step
            const float* nx = cost + (int64_t)(t + 1) * K;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int k = i * 64 + lane;
                cn[i] = k < K ? nx[k] : INFINITY;
            }
        }
        seg_wave_min<W>(r, lane, m, a);
        acc = acc + m;
        uint64_t word = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            bool stay;
            r[i] = seg_step(r[i], m, lam, c[i], &stay);
            const uint64_t bits = __ballot(stay ? 1 : 0);
            if (lane == i) word = bits;
        }
        uint64_t* row = back + (int64_t)t * (Wk + 1);
        if (lane < Wk) row[lane] = word;
        if (lane == 0) row[Wk] = (uint64_t)a;
    }
    seg_wave_min<W>(r, lane, m, a);
    const float total = acc + m;
    __threadfence();                                                             // the back words, before lane 0 reads them
    int64_t* codes = p.codes + rec.first_frame;
    if (lane == 0) {
        p.cost[u] = total;
        p.n_seg[u] = seg_walk(back, Wk, T, K, a, codes);
        if (!isfinite(total)) atomicAdd(p.n_bad, 1u);
    }
    if (!p.dist) return;
    __threadfence();                                                             // the codes, before the other lanes read them
    float* dist = p.dist + rec.first_frame;
    for (int t = lane; t < T; t += 64) {
        int64_t k = codes[t];
        if (k < 0 || k >= K) k = 0;
        dist[t] = cost[(int64_t)t * K + k];
    }
}

// ---- the launcher ----------------------------------------------------------------------------------------------------------
template <int DR>
static void seg_launch_cost(const aew_code_segment_t& p, int64_t n_rows, hipStream_t st) {
    const dim3 grid((unsigned)((n_rows + SEG_SLAB - 1) / SEG_SLAB), (unsigned)((p.K + SEG_GROUP - 1) / SEG_GROUP));
    float* cost = (float*)p.ws;
    if (DR > 0 && p.d == DR)
        hipLaunchKernelGGL((k_seg_cost<DR, true>), grid, dim3(SEG_GROUP), 0, st, p.frames, p.emb, cost, n_rows, p.K, p.d, p.d_pitch, p.metric);
    else
        hipLaunchKernelGGL((k_seg_cost<DR, false>), grid, dim3(SEG_GROUP), 0, st, p.frames, p.emb, cost, n_rows, p.K, p.d, p.d_pitch, p.metric);
}

static int launch_code_segment(const aew_code_segment_t& p, hipStream_t st) {
    int64_t n_rows = 0;
    int rc = seg_check(p, false, &n_rows);
    if (rc) return rc;
    if (p.U == 0) return 0;
    if (n_rows > 0) {
        if (n_rows > (int64_t)SEG_SLAB * 0x7fffffff) return AEW_E_ARG;
        if (p.d <= 8) seg_launch_cost<8>(p, n_rows, st);
        else if (p.d <= 16) seg_launch_cost<16>(p, n_rows, st);
        else if (p.d <= 32) seg_launch_cost<32>(p, n_rows, st);
        else if (p.d <= 64) seg_launch_cost<64>(p, n_rows, st);
        else seg_launch_cost<0>(p, n_rows, st);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    const dim3 g((unsigned)p.U), blk(64);
    const int W = seg_words(p.K);
    if (W <= 1) hipLaunchKernelGGL(k_seg_scan<1>, g, blk, 0, st, p, n_rows);
    else if (W <= 2) hipLaunchKernelGGL(k_seg_scan<2>, g, blk, 0, st, p, n_rows);
    else if (W <= 4) hipLaunchKernelGGL(k_seg_scan<4>, g, blk, 0, st, p, n_rows);
    else if (W <= 8) hipLaunchKernelGGL(k_seg_scan<8>, g, blk, 0, st, p, n_rows);
    else if (W <= 16) hipLaunchKernelGGL(k_seg_scan<16>, g, blk, 0, st, p, n_rows);
    else if (W <= 32) hipLaunchKernelGGL(k_seg_scan<32>, g, blk, 0, st, p, n_rows);
    else hipLaunchKernelGGL(k_seg_scan<64>, g, blk, 0, st, p, n_rows);
    return (int)hipGetLastError();
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------
extern "C" int aew_segment_host(const aew_code_segment_t* pp) {
    if (!pp) return AEW_E_ARG;
    const aew_code_segment_t& p = *pp;
    int64_t n_rows = 0;
    const int rc = seg_check(p, true, &n_rows);
    if (rc) return rc;
    if (p.U == 0) return 0;
    const int K = p.K, d = p.d, W = seg_words(K);
    float* cost = (float*)p.ws;
    uint64_t* back_all = (uint64_t*)((char*)p.ws + seg_cost_bytes(n_rows, K));
    std::vector<float> sq(K), r(K);
    for (int k = 0; k < K; ++k) {
        float qq = 0.f;
        for (int j = 0; j < d; ++j) qq = seg_fma(p.emb[(int64_t)k * d + j], p.emb[(int64_t)k * d + j], qq);
        sq[k] = sqrtf(qq);
    }
    for (int64_t f = 0; f < n_rows; ++f) {                                       // what k_seg_cost leaves in the workspace
        const float* z = p.frames + f * p.d_pitch;
        float zz = 0.f;
        if (p.metric == 0) for (int j = 0; j < d; ++j) zz = seg_fma(z[j], z[j], zz);
        const float zn = sqrtf(zz);
        for (int k = 0; k < K; ++k) {
            const float* e = p.emb + (int64_t)k * d;
            float dd = 0.f;
            for (int j = 0; j < d; ++j) dd = seg_dd(z[j], e[j], dd);
            cost[f * K + k] = seg_cost_of(dd, zn, sq[k], p.metric);
        }
    }
    for (int u = 0; u < p.U; ++u) {                                              // what one wave of k_seg_scan does
        const aew_seg_utt_t& rec = p.table_host[u];
        const int T = rec.n_frames;
        if (T == 0) { p.cost[u] = 0.f; p.n_seg[u] = 0; continue; }
        const float* c = cost + rec.first_frame * K;
        uint64_t* back = back_all + rec.back_base;
        for (int k = 0; k < K; ++k) r[k] = c[k];
        float acc = 0.f, m;
        int a;
        auto take_min = [&]() {
            float best = INFINITY;
            int bi = 0x7fffffff;
            for (int k = 0; k < K; ++k)
                if (r[k] < best) { best = r[k]; bi = k; }                        // ascending k: what seg_beats orders the lanes by
            m = best;
            a = bi == 0x7fffffff ? 0 : bi;
        };
        for (int t = 1; t < T; ++t) {
            take_min();
            acc = acc + m;
            uint64_t* row = back + (int64_t)t * (W + 1);
            for (int i = 0; i < W; ++i) row[i] = 0;
            for (int k = 0; k < K; ++k) {
                bool stay;
                r[k] = seg_step(r[k], m, rec.lam, c[(int64_t)t * K + k], &stay);
                if (stay) row[k >> 6] |= (uint64_t)1 << (k & 63);
            }
            row[W] = (uint64_t)a;
        }
        take_min();
        const float total = acc + m;
        int64_t* codes = p.codes + rec.first_frame;
        p.cost[u] = total;
        p.n_seg[u] = seg_walk(back, W, T, K, a, codes);
        if (!std::isfinite(total)) *p.n_bad += 1u;
        if (p.dist)
            for (int t = 0; t < T; ++t) p.dist[rec.first_frame + t] = c[(int64_t)t * K + codes[t]];
    }
    return 0;
}
