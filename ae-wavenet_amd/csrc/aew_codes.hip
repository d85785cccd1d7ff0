// aew_codes.hip — code sequences as data: codes -> codebook rows (aew_code_lookup_t, the inverse of the nearest-code
// search on its zq output) and the run-length collapse of code rows into units (aew_code_runs_t).  Byte movers and
// integer work: no floating point arithmetic, no waiting on another workgroup.
#include "aew_common.h"

// =============================================================================================
// lookup: zq[q][0:d) = emb[ind[q]][0:d), zq[q][d:d_pitch) = 0.  An index outside [0, K) is tested BEFORE any address is
// formed from it: its row is zeros and the thread that owns channel 0 of the row counts it in *bad.
// VEC: one thread per 4 channels (16-byte accesses; d and d_pitch multiples of 4, emb and zq 16-byte aligned);
// otherwise one thread per channel.
// =============================================================================================
template <bool VEC>
__global__ __launch_bounds__(256) void k_code_lookup(const aew_code_lookup_t p) {
    constexpr int W = VEC ? 4 : 1;
    const int per_row = p.d_pitch / W;
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (int64_t)p.Q * per_row) return;
    const int q = (int)(item / per_row);
    const int j = (int)(item - (int64_t)q * per_row) * W;            // first channel of this thread
    const int64_t k = p.ind[q];
    const bool ok = k >= 0 && k < (int64_t)p.K;
    if (!ok && j == 0 && p.bad) atomicAdd(p.bad, 1u);
    float* dst = p.zq + (int64_t)q * p.d_pitch + j;
    if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && j < p.d) v = *reinterpret_cast<const float4*>(p.emb + k * p.d + j);
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        float v = 0.f;
        if (ok && j < p.d) v = p.emb[k * p.d + j];
        *dst = v;
    }
}

static int launch_code_lookup(const aew_code_lookup_t& p, hipStream_t st) {
    if (p.Q < 1 || p.K < 1 || p.d < 1 || p.d_pitch < p.d || !p.ind || !p.emb || !p.zq) return AEW_E_ARG;
    if (((uintptr_t)p.ind & 7) || (((uintptr_t)p.emb | (uintptr_t)p.zq | (uintptr_t)p.bad) & 3)) return AEW_E_ALIGN;
    const bool vec = p.d % 4 == 0 && p.d_pitch % 4 == 0 && (((uintptr_t)p.emb | (uintptr_t)p.zq) & 15) == 0;
    const int64_t items = (int64_t)p.Q * (p.d_pitch / (vec ? 4 : 1));
    const int64_t blocks = (items + 255) / 256;
    if (blocks > 0x7fffffff) return AEW_E_ARG;
    hipLaunchKernelGGL(vec ? k_code_lookup<true> : k_code_lookup<false>, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return (int)hipGetLastError();
}

// =============================================================================================
// runs: one workgroup per row.  A chunk is AEW_RUNS_CHUNK = 1024 positions: four slices of 256, thread i of the block owns
// position i of every slice, and all loads of a chunk are issued before anything waits for them (the row is walked by ONE
// workgroup, so the loop is a chain of memory latencies: four positions per thread make it four times shorter).
// start(t) = t == 0 || ind[t] != ind[t - 1].  Inside a wave the ballot of `start` gives a start's rank (popcount of the
// lanes below it) and the position of the start before it (highest set lane below it); every (slice, wave) segment leaves
// its count and its last start in LDS, and every thread folds the segments in front of its own - and the carry of the
// chunks before - in ascending order of position.  A start that opens run r writes units[r] and closes run r - 1:
// lengths[r - 1] = t - (start of run r - 1).  The last run is closed behind the loop, then the tail r >= n_runs is
// filled.  Every output element has exactly one writer and nothing that was written is read back.
// =============================================================================================
#define AEW_RUNS_THREADS 256
#define AEW_RUNS_SLICES 4
#define AEW_RUNS_CHUNK (AEW_RUNS_THREADS * AEW_RUNS_SLICES)
__global__ __launch_bounds__(AEW_RUNS_THREADS) void k_code_runs(const aew_code_runs_t p) {
    constexpr int NW = AEW_RUNS_THREADS / AEW_WAVE, U = AEW_RUNS_SLICES;
    __shared__ int s_cnt[U][NW];
    __shared__ int s_last[U][NW];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (AEW_WAVE - 1), wave = tid / AEW_WAVE;
    const int N = p.N;
    const int64_t* row = p.ind + (int64_t)b * p.ind_pitch;
    int64_t* units = p.units + (int64_t)b * N;
    int32_t* lengths = p.lengths + (int64_t)b * N;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    int runs = 0;                // runs opened in the chunks before this one
    int last = 0;                // position of the last start in them (position 0 always starts a run)
    for (int64_t c = 0; c < N; c += AEW_RUNS_CHUNK) {
        int64_t v[U], pv[U];
        bool valid[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {                                 // every load of the chunk first
            const int64_t t = c + j * AEW_RUNS_THREADS + tid;
            valid[j] = t < N;
            v[j] = valid[j] ? row[t] : 0;
            pv[j] = (valid[j] && t > 0) ? row[t - 1] : 0;
        }
        unsigned long long bal[U];
        bool start[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int64_t t = c + j * AEW_RUNS_THREADS + tid;
            start[j] = valid[j] && (t == 0 || v[j] != pv[j]);
            bal[j] = __ballot(start[j]);
            if (lane == 0) {
                s_cnt[j][wave] = __popcll(bal[j]);
                s_last[j][wave] = bal[j] ? (int)(t + 63 - __clzll((long long)bal[j])) : -1;      // (t = lane 0's position)
            }
        }
        __syncthreads();
        int acc = runs, tail = last;                                  // carry in front of segment (j, w), ascending
        int off[U], prev[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (w == wave) { off[j] = acc; prev[j] = tail; }
                const int l = s_last[j][w];
                acc += s_cnt[j][w];
                if (l >= 0) tail = l;
            }
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (start[j]) {
                const int t = (int)(c + j * AEW_RUNS_THREADS + tid);
                const unsigned long long below = bal[j] & lanes_below;
                const int r = off[j] + __popcll(below);
                const int before = below ? t - lane + 63 - __clzll((long long)below) : prev[j];
                units[r] = v[j];
                if (r > 0) lengths[r - 1] = t - before;
            }
        }
        runs = acc;
        last = tail;
        __syncthreads();                                              // s_cnt / s_last are rewritten by the next chunk
    }
    if (tid == 0) {
        lengths[runs - 1] = N - last;
        p.n_runs[b] = runs;
    }
    for (int64_t r = (int64_t)runs + tid; r < N; r += AEW_RUNS_THREADS) {
        units[r] = -1;
        lengths[r] = 0;
    }
}

static int launch_code_runs(const aew_code_runs_t& p, hipStream_t st) {
    if (p.B < 1 || p.N < 1 || p.ind_pitch < p.N || !p.ind || !p.units || !p.lengths || !p.n_runs) return AEW_E_ARG;
    if ((((uintptr_t)p.ind | (uintptr_t)p.units) & 7) || (((uintptr_t)p.lengths | (uintptr_t)p.n_runs) & 3)) return AEW_E_ALIGN;
    hipLaunchKernelGGL(k_code_runs, dim3((unsigned)p.B), dim3(AEW_RUNS_THREADS), 0, st, p);
    return (int)hipGetLastError();
}
