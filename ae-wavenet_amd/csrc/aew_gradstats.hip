// aew_gradstats.hip — gradient noise statistics on the flat parameter-sized buffers: AEW_OP_GRAD_WELFORD folds one
// gradient sample into a running mean / sum of squared deviations, AEW_OP_SEG_SELECT takes exact k-th smallest values per
// tensor (aew_grad_welford_t / aew_seg_select_t in aewavenet.h state the contracts; the reference: grad_analysis.py
// mu_s_incr, quantiles, grad_stats).  Part of the library's one translation unit (aewavenet.hip includes it behind
// aew_ops.hip, whose chunk table, zero launch and block sum it uses).
#pragma once
#include "aew_common.h"

// =============================================================================================
// Welford (grad_analysis.py:32-39)
// =============================================================================================
// One element's update.  The plain and the chunked launch both go through this function, vector and scalar paths alike.
// Round-to-nearest intrinsics: nothing is contracted, the division is a true fp32 division.
template <bool FIRST>
__device__ __forceinline__ void welford_elem(const float g, float& mu, float& s, const float divisor) {
    if (FIRST) { mu = g; s = 0.f; return; }
    const float d = __fsub_rn(g, mu);
    const float mu2 = __fadd_rn(mu, __fdiv_rn(d, divisor));
    s = __fadd_rn(s, __fmul_rn(d, __fsub_rn(g, mu2)));
    mu = mu2;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_grad_welford(const aew_grad_welford_t p) {
    const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 >= p.n) return;
    if (i4 + 4 <= p.n) {
        const float4 g = *reinterpret_cast<const float4*>(p.g + i4);
        float4 mu, s;
        if (!FIRST) { mu = *reinterpret_cast<const float4*>(p.mu + i4); s = *reinterpret_cast<const float4*>(p.s + i4); }
        const float* gp = &g.x; float* mp = &mu.x; float* sp = &s.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) welford_elem<FIRST>(gp[r], mp[r], sp[r], p.divisor);
        *reinterpret_cast<float4*>(p.mu + i4) = mu;
        *reinterpret_cast<float4*>(p.s + i4) = s;
    } else {
        for (int64_t i = i4; i < p.n; ++i) {
            float mu = 0.f, s = 0.f;
            if (!FIRST) { mu = p.mu[i]; s = p.s[i]; }
            welford_elem<FIRST>(p.g[i], mu, s, p.divisor);
            p.mu[i] = mu; p.s[i] = s;
        }
    }
}

// The chunked launch: one block per chunk of the host's chunk table (k_adam_uw's shape).  The block updates the chunk and
// the pad elements behind it, and sums s' and mu'^2 over the chunk's own elements in fp64: per thread one chain per sum
// (float4 rounds ascending, components ascending), gn_block_sum (butterfly inside the wave, waves ascending).
template <bool FIRST>
__global__ __launch_bounds__(256) void k_grad_welford_chunks(const aew_grad_welford_t p) {
    constexpr int IT = AEW_UW_CHUNK / 1024;
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const aew_uw_chunk_t c = p.chunks[blockIdx.x];
    const int64_t e_sum = min(c.off + (int64_t)c.len, p.n);
    const int64_t e_upd = min(c.off + (int64_t)((c.len + 3) & ~3), p.n);
    double ss = 0.0, sm = 0.0;
    float4 g[IT], mu[IT], s[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {                  // every load of the block in flight first
        const int64_t i4 = c.off + (int64_t)(it * 256 + tid) * 4;
        if (i4 + 4 <= e_upd) {
            g[it] = *reinterpret_cast<const float4*>(p.g + i4);
            if (!FIRST) { mu[it] = *reinterpret_cast<const float4*>(p.mu + i4); s[it] = *reinterpret_cast<const float4*>(p.s + i4); }
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int64_t i4 = c.off + (int64_t)(it * 256 + tid) * 4;
        if (i4 + 4 <= e_upd) {
            const float* gp = &g[it].x; float* mp = &mu[it].x; float* sp = &s[it].x;
#pragma unroll
            for (int r = 0; r < 4; ++r) welford_elem<FIRST>(gp[r], mp[r], sp[r], p.divisor);
            *reinterpret_cast<float4*>(p.mu + i4) = mu[it];
            *reinterpret_cast<float4*>(p.s + i4) = s[it];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i4 + r < e_sum) { ss += (double)sp[r]; sm += (double)mp[r] * (double)mp[r]; }
        } else if (i4 < e_upd) {                       // n % 4 elements at the very end of the buffer
            for (int64_t i = i4; i < e_upd; ++i) {
                float m1 = 0.f, s1 = 0.f;
                if (!FIRST) { m1 = p.mu[i]; s1 = p.s[i]; }
                welford_elem<FIRST>(p.g[i], m1, s1, p.divisor);
                p.mu[i] = m1; p.s[i] = s1;
                if (i < e_sum) { ss += (double)s1; sm += (double)m1 * (double)m1; }
            }
        }
    }
    ss = gn_block_sum(ss, sh);
    sm = gn_block_sum(sm, sh);
    if (tid == 0) {                                    // the chunk's only writer: plain stores
        p.part[2 * (int64_t)blockIdx.x] = ss;
        p.part[2 * (int64_t)blockIdx.x + 1] = sm;
    }
}

static bool gs_overlap(const void* a, const void* b, int64_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y ? x + (uintptr_t)bytes > y : y + (uintptr_t)bytes > x;
}

static int launch_grad_welford(const aew_grad_welford_t& p, hipStream_t st) {
    if (p.n < 0 || (p.n > 0 && (!p.g || !p.mu || !p.s))) return AEW_E_ARG;
    if (p.first != 0 && p.first != 1) return AEW_E_ARG;
    if (!p.first && !(p.divisor > 0.f)) return AEW_E_ARG;
    if (p.n > 0 && (gs_overlap(p.g, p.mu, 4 * p.n) || gs_overlap(p.g, p.s, 4 * p.n) || gs_overlap(p.mu, p.s, 4 * p.n))) return AEW_E_ARG;
    if (p.part) {
        // the chunks (+ the pad elements behind each) must cover [0, n) without a gap: an element outside every chunk
        // would miss its update, and mu / s would depend on whether the sums were asked for
        const aew_uw_chunk_t* ch = p.chunks_host;
        if (!p.chunks || !ch || p.n_chunks < 1 || p.n_chunks > 0x7fffffff || p.n < 1) return AEW_E_ARG;
        auto pad_end = [&](int64_t c) { return ch[c].off + ((ch[c].len + 3) & ~3); };
        if (ch[0].off != 0) return AEW_E_ARG;
        for (int64_t c = 0; c < p.n_chunks; ++c) {
            if (ch[c].len < 1 || ch[c].len > AEW_UW_CHUNK || (ch[c].off & 3)) return AEW_E_ARG;
            if (c + 1 < p.n_chunks ? pad_end(c) != ch[c + 1].off : pad_end(c) < p.n) return AEW_E_ARG;
        }
        if (ch[p.n_chunks - 1].off >= p.n) return AEW_E_ARG;
    }
    if (((uintptr_t)p.g | (uintptr_t)p.mu | (uintptr_t)p.s | (uintptr_t)p.part) & 15) return AEW_E_ALIGN;
    if (p.n == 0) return 0;
    if (p.part) {
        auto k = p.first ? k_grad_welford_chunks<true> : k_grad_welford_chunks<false>;
        hipLaunchKernelGGL(k, dim3((unsigned)p.n_chunks), dim3(256), 0, st, p);
    } else {
        const int64_t blocks = cdiv64((p.n + 3) / 4, 256);
        if (blocks > 0x7fffffff) return AEW_E_ARG;
        auto k = p.first ? k_grad_welford<true> : k_grad_welford<false>;
        hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(256), 0, st, p);
    }
    return (int)hipGetLastError();
}

// =============================================================================================
// exact k-th smallest per tensor (grad_analysis.py:42-50): radix select over the order key, four passes of 8 bits
// =============================================================================================
// ---- the order key, ONE definition for the kernels and for aew_select_key (the CPU tests run this very code)
__host__ __device__ __forceinline__ uint32_t select_key(const float s, const uint32_t bits) {
    return s >= 0.f ? (bits & 0x7fffffffu) : 0xffffffffu;          // -0 -> +0; negative or NaN: behind everything
}
extern "C" int aew_select_key(uint32_t bits, uint32_t* key) {
    if (!key) return AEW_E_ARG;
    union { uint32_t u; float f; } v;
    v.u = bits;
    *key = select_key(v.f, bits);
    return 0;
}

#define AEW_SELECT_BINS 256
// scratch: hist uint32 [P][Q][256], then prefix uint32 [P][Q], then rank uint32 [P][Q] (0 = nothing left to find)
static int64_t select_scratch_words(int64_t P, int64_t Q) { return P * Q * (AEW_SELECT_BINS + 2); }

extern "C" int aew_seg_select_size(const aew_seg_select_t* p, int64_t* bytes) {
    if (!p || !bytes || p->n_tensors < 1 || p->Q < 1 || p->Q > AEW_SELECT_MAX_Q) return AEW_E_ARG;
    *bytes = (select_scratch_words(p->n_tensors, p->Q) * 4 + 15) & ~(int64_t)15;
    return 0;
}

// leader[q]: the lowest rank slot of the tensor that is alive and carries the same prefix - slots with one prefix share
// one histogram (all of them in the first pass, equal ranks in every pass).  -1: the slot is dead.
__device__ __forceinline__ void select_leaders(const int Q, const uint32_t* pre, const uint32_t* rank, int* lead) {
    for (int q = 0; q < Q; ++q) {
        int l = -1;
        if (rank[q] != 0u) {
            l = q;
            for (int j = q - 1; j >= 0; --j)
                if (rank[j] != 0u && pre[j] == pre[q]) l = j;
        }
        lead[q] = l;
    }
}

__global__ void k_select_init(const aew_seg_select_t p, uint32_t* prefix, uint32_t* rank) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_tensors * p.Q) return;
    const int k = p.k[i];
    prefix[i] = 0u;
    rank[i] = k > 0 ? (uint32_t)k : 0u;
}

// One block per chunk: count, per live prefix of the chunk's tensor, the next 8 key bits of the elements under it.
__global__ __launch_bounds__(256) void k_select_pass(const aew_seg_select_t p, uint32_t* hist, const uint32_t* prefix,
                                                     const uint32_t* rank, const int pass) {
    constexpr int IT = AEW_UW_CHUNK / 1024;
    __shared__ uint32_t h[AEW_SELECT_MAX_Q * AEW_SELECT_BINS];
    __shared__ uint32_t s_pre[AEW_SELECT_MAX_Q], s_rank[AEW_SELECT_MAX_Q];
    __shared__ int s_lead[AEW_SELECT_MAX_Q];
    const int tid = threadIdx.x, Q = p.Q;
    const aew_uw_chunk_t c = p.chunks[blockIdx.x];
    const int t = c.tensor;
    if (t < 0 || t >= p.n_tensors) return;             // (uniform: a table that names no tensor of this op)
    const int len = c.len < AEW_UW_CHUNK ? c.len : AEW_UW_CHUNK;
    if (tid < Q) { s_pre[tid] = prefix[t * Q + tid]; s_rank[tid] = rank[t * Q + tid]; }
    for (int i = tid; i < Q * AEW_SELECT_BINS; i += 256) h[i] = 0u;
    __syncthreads();
    if (tid == 0) select_leaders(Q, s_pre, s_rank, s_lead);
    __syncthreads();
    const int sh_hi = pass ? 32 - 8 * pass : 0, sh_bin = 24 - 8 * pass;      // (pass 0 has no prefix to compare)
    const float* x = p.s + c.off;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int i4 = (it * 256 + tid) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (i4 + 4 <= len) {
            const float4 f = *reinterpret_cast<const float4*>(x + i4);       // c.off is a multiple of 4
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
            for (int r = 0; r < 4; ++r)
                if (i4 + r < len) v[r] = x[i4 + r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool act = i4 + r < len;
            const uint32_t key = select_key(v[r], __float_as_uint(v[r]));
            const uint32_t bin = (key >> sh_bin) & 255u;
            for (int q = 0; q < Q; ++q) {              // (uniform)
                if (s_lead[q] != q) continue;
                const bool m = act && (pass == 0 || (key >> sh_hi) == s_pre[q]);
                // a wave whose matching lanes all hit one bin adds their number once (the common case in the high bytes)
                const unsigned long long mask = __ballot(m);
                if (mask == 0ull) continue;
                const int leader_lane = __ffsll((long long)mask) - 1;
                const uint32_t b0 = (uint32_t)__shfl((int)bin, leader_lane);
                if (__ballot(m && bin != b0) == 0ull) {
                    if ((tid & 63) == leader_lane) atomicAdd(&h[q * AEW_SELECT_BINS + b0], (uint32_t)__popcll(mask));
                } else if (m)
                    atomicAdd(&h[q * AEW_SELECT_BINS + bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < Q * AEW_SELECT_BINS; i += 256) {
        const int q = i >> 8;
        if (s_lead[q] == q && h[i] != 0u) atomicAdd(&hist[((int64_t)t * Q + q) * AEW_SELECT_BINS + (i & 255)], h[i]);
    }
}

// One block of 256 threads per tensor: per rank slot, find the bin that holds the rank, narrow the prefix, reduce the
// rank to its place inside the bin; clear the histograms for the next pass.  The last pass writes the outputs.
__global__ __launch_bounds__(256) void k_select_pick(const aew_seg_select_t p, uint32_t* hist, uint32_t* prefix, uint32_t* rank,
                                                     const int pass) {
    __shared__ uint32_t s_pre[AEW_SELECT_MAX_Q], s_rank[AEW_SELECT_MAX_Q], s_npre[AEW_SELECT_MAX_Q], s_nrank[AEW_SELECT_MAX_Q];
    __shared__ int s_lead[AEW_SELECT_MAX_Q];
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, Q = p.Q, t = blockIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < Q) { s_pre[tid] = prefix[t * Q + tid]; s_rank[tid] = rank[t * Q + tid]; s_npre[tid] = 0u; s_nrank[tid] = 0u; }
    __syncthreads();
    if (tid == 0) select_leaders(Q, s_pre, s_rank, s_lead);
    __syncthreads();
    for (int q = 0; q < Q; ++q) {                      // (uniform)
        const int l = s_lead[q];
        if (l < 0) continue;
        const uint32_t cnt = hist[((int64_t)t * Q + l) * AEW_SELECT_BINS + tid];
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= o) incl += up;
        }
        __syncthreads();                               // (the previous slot's readers are done with wsum)
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t base = 0u;
        for (int j = 0; j < w; ++j) base += wsum[j];
        const uint32_t excl = base + incl - cnt, k = s_rank[q];
        if (excl < k && k <= excl + cnt) {             // exactly one bin holds the rank (none: the rank exceeds the length)
            s_npre[q] = (s_pre[q] << 8) | (uint32_t)tid;
            s_nrank[q] = k - excl;
        }
    }
    __syncthreads();
    for (int q = 0; q < Q; ++q)
        if (s_lead[q] == q) hist[((int64_t)t * Q + q) * AEW_SELECT_BINS + tid] = 0u;
    if (tid < Q) {
        prefix[t * Q + tid] = s_npre[tid];
        rank[t * Q + tid] = s_nrank[tid];
        if (pass == 3) {
            const uint32_t key = s_npre[tid];
            float o = __uint_as_float(0x7fc00000u);    // NaN: the NaN key, an empty tensor, a rank outside 1 .. len
            if (s_nrank[tid] != 0u && key != 0xffffffffu) {
                const float v = __uint_as_float(key);
                o = p.raw ? v : sqrtf(__fdiv_rn(v, p.denom));      // (sqrtf is the IEEE-rounded root here)
            }
            p.out[t * Q + tid] = o;
        }
    }
}

static int launch_seg_select(const aew_seg_select_t& p, hipStream_t st) {
    if (p.Q < 1 || p.Q > AEW_SELECT_MAX_Q || p.n_tensors < 1 || p.n_chunks < 0 || p.n_chunks > 0x7fffffff) return AEW_E_ARG;
    if ((int64_t)p.n_tensors * p.Q > 0x7fffffff / (AEW_SELECT_BINS + 2)) return AEW_E_ARG;
    if (!p.k || !p.out || !p.scratch || (p.n_chunks > 0 && (!p.s || !p.chunks))) return AEW_E_ARG;
    if (p.raw != 0 && p.raw != 1) return AEW_E_ARG;
    if (!p.raw && !(p.denom > 0.f)) return AEW_E_ARG;
    if (((uintptr_t)p.s | (uintptr_t)p.scratch) & 15) return AEW_E_ALIGN;
    if ((uintptr_t)p.chunks & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.k | (uintptr_t)p.out) & 3) return AEW_E_ALIGN;
    const int64_t PQ = (int64_t)p.n_tensors * p.Q;
    uint32_t* hist = reinterpret_cast<uint32_t*>(p.scratch);
    uint32_t* prefix = hist + PQ * AEW_SELECT_BINS;
    uint32_t* rank = prefix + PQ;
    aew_zero_t z;
    z.ptr = p.scratch; z.bytes = PQ * AEW_SELECT_BINS * 4;          // (a multiple of 16)
    if (int rc = launch_zero(z, st)) return rc;
    hipLaunchKernelGGL(k_select_init, dim3((unsigned)cdiv64(PQ, 256)), dim3(256), 0, st, p, prefix, rank);
    for (int pass = 0; pass < 4; ++pass) {
        if (p.n_chunks > 0)
            hipLaunchKernelGGL(k_select_pass, dim3((unsigned)p.n_chunks), dim3(256), 0, st, p, hist, (const uint32_t*)prefix,
                               (const uint32_t*)rank, pass);
        hipLaunchKernelGGL(k_select_pick, dim3((unsigned)p.n_tensors), dim3(256), 0, st, p, hist, prefix, rank, pass);
    }
    return (int)hipGetLastError();
}
