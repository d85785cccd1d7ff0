// aew_align.hip — AEW_OP_SEQ_ALIGN: batched dynamic time warping over fp32 frames and the Levenshtein distance of int64
// symbol strings, one WAVEFRONT per pair (aewavenet.h states the rule and the records' checks).
//
// Shape.  A wave walks its pair in strips of 64 A frames: lane r owns row i0 + r.  Inside a strip it sweeps the
// anti-diagonals along j - at step t lane r is at column j = t - r - so that C / S of the upper and the diagonal neighbour
// are the values the lane below held one and two steps ago (one DPP move per value, the diagonal is the previous
// step's upper value kept in a register) and the left neighbour is the lane's own last value.  The strip's bottom row goes
// to the workspace and comes back as the next strip's top row, 64 columns per load, handed to lane 0 by a uniform-index
// lane read.  DTW alternates two phases per 64 columns: (A) the local distances of the 64 columns for all 64 rows - lane l
// loads B frame j0 + l into registers, column jj's frame reaches the wave by lane reads at the uniform index jj, the lane's
// A row sits in registers for D <= 64, so the column loop touches no memory - into a per-lane ring of 128 columns in LDS
// (ring[column & 127][lane]: a lane reads back only what it wrote itself, bank = lane, no conflict); (B) the 64 sweep
// steps that have all their columns by then.  EDIT needs no ring: the B symbols travel up the lanes, one lane per step.
//
// The DTW strip loop is ONE device function, align_sweep<DR, SUB>: k_align_dtw calls it with SUB = false, k_search_sweep
// (aew_search.hip, subsequence DTW) with SUB = true; what only one of the two carries is compiled out of the other.
// Phase (A) is a function of its own, align_fill_ring<DR>: k_discover_sweep (aew_discover.hip, local-alignment DTW) runs
// a sibling sweep with another recurrence over the same ring.  The two strip loops stay apart: written once over a generic
// carried cell, the 64-step loop of search and discover compiled to another instruction order and measured 1 - 3 %
// slower, and as one frame around a step loop per op DTW's loop grew by a quarter (profiles/search.txt).  The three ops
// share the sweep kernels' prologue (align_wave_of), the device pair loader (seq_load_pair), the host checks of the
// fields their records have in common (align_check_record) with the workspace's width from each op's carried words
// (align_ws_col), the ladder D -> DR (align_dispatch_D) and the launch of a sweep with the kernel behind it
// (align_launch_sweep).
//
// Nothing here waits on another wave: no __syncthreads (the waves of a block share nothing), no flag, no atomic but the
// count of pairs that are not finite.  The path kernel is a second launch behind the first on the same stream.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_score.hip).
#pragma once
#include "aew_common.h"
#include <math.h>
#include <type_traits>

#define AEW_ALIGN_WAVES 2          // waves (pairs) per workgroup of the DTW kernel: 2 x 32 KiB of ring = 64 KiB of LDS
#define AEW_ALIGN_EDIT_WAVES 4     // the EDIT kernel holds no LDS
#define AEW_ALIGN_RING 128         // columns of local distances a lane keeps: the 64 being swept + the 64 being filled

// ---- the records' checks, ONE definition for the launcher (host copies) and the kernels (device copies) ---------------
// 1 if every element (i < len, k < D) of the sequence lies inside [0, n_elems)
__host__ __device__ __forceinline__ int align_seq_ok(const aew_align_seq_t& s, int D, int64_t n_elems) {
    if (s.len < 0 || s.len > AEW_ALIGN_MAX_LEN) return 0;
    if (s.len == 0) return 1;
    const int64_t lim = (int64_t)1 << 40;
    if (s.base < 0 || s.base >= n_elems || s.frame_stride < 0 || s.frame_stride > lim || s.chan_stride < 0 || s.chan_stride > lim)
        return 0;
    const int64_t last = s.base + (int64_t)(s.len - 1) * s.frame_stride + (int64_t)(D - 1) * s.chan_stride;   // < 2^50 + 2^60 + 2^48
    return last < n_elems;
}
__host__ __device__ __forceinline__ int align_pair_ok(int a, int b, int n_a, int n_b) {
    return a >= 0 && a < n_a && b >= 0 && b < n_b;
}
// 1 if the pair's n * m back bytes and - where a path is kept - its n + m - 1 path entries lie inside their buffers
__host__ __device__ __forceinline__ int align_room_ok(const aew_align_pair_t& p, int n, int m, int64_t n_back, bool path, int64_t n_path) {
    if (n == 0 || m == 0) return 1;
    const int64_t cells = (int64_t)n * m, cap = (int64_t)n + m - 1;
    if (p.back_base < 0 || cells > n_back || p.back_base > n_back - cells) return 0;
    if (path && (p.path_base < 0 || cap > n_path || p.path_base > n_path - cap)) return 0;
    return 1;
}

// what a wave needs of its pair, read and checked from the device copies; ok = 0: the pair is left alone.  Rec is
// aew_seq_align_t or aew_seq_search_t, Pair its pair record; each op puts only its own room check on top
template <class Pair>
struct seq_pair_view {
    Pair pr;
    aew_align_seq_t sa, sb;
    int ok;
};
template <class Rec>
__device__ __forceinline__ auto seq_load_pair(const Rec& p, int pi, int64_t wstride) {
    seq_pair_view<std::decay_t<decltype(p.pairs[0])>> v;
    v.ok = 0;
    v.pr = p.pairs[pi];
    if (!align_pair_ok(v.pr.a, v.pr.b, p.n_a, p.n_b)) return v;
    v.sa = p.seq_a[v.pr.a];
    v.sb = p.seq_b[v.pr.b];
    if (!align_seq_ok(v.sa, p.D, p.n_feat_a) || !align_seq_ok(v.sb, p.D, p.n_feat_b)) return v;
    if (v.sa.len > 64 && v.sb.len > 0 && (!p.ws || v.sb.len > wstride)) return v;   // (the tables changed under a captured graph)
    v.ok = 1;
    return v;
}
typedef seq_pair_view<aew_align_pair_t> align_pair_view;
__device__ __forceinline__ align_pair_view align_load_pair(const aew_seq_align_t& p, int pi, int64_t wstride) {
    align_pair_view v = seq_load_pair(p, pi, wstride);
    if (v.ok && p.back && !align_room_ok(v.pr, v.sa.len, v.sb.len, p.n_back, p.path != nullptr, p.n_path)) v.ok = 0;
    return v;
}

// ---- moving a value between the lanes of the wave without the LDS crossbar -----------------------------------------------
// the value lane l - 1 holds (lane 0: 0): one DPP move, wave_shr:1
__device__ __forceinline__ int align_up1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float align_up1(float v) { return __builtin_bit_cast(float, align_up1(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ int64_t align_up1(int64_t v) {
    const uint32_t lo = (uint32_t)align_up1((int)(uint32_t)v), hi = (uint32_t)align_up1((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the value lane l holds, l wave-uniform: v_readlane_b32
__device__ __forceinline__ int align_lane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float align_lane(float v, int l) { return __builtin_bit_cast(float, align_lane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ int64_t align_lane(int64_t v, int l) {
    const uint32_t lo = (uint32_t)align_lane((int)(uint32_t)v, l), hi = (uint32_t)align_lane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---- the DTW sweep, for AEW_OP_SEQ_ALIGN and AEW_OP_SEQ_SEARCH -------------------------------------------------------------
// A carried cell is one float and `words` int words - DTW's S; search's S, B; discover's S, R, O - and the workspace holds
// a boundary row as 1 + words planes of n_pairs * wstride words: plane 0 the float, plane 1 + w word w.  -> the bytes a
// pair and column take of it
#define AEW_ALIGN_WORDS 1
#define AEW_SEARCH_WORDS 2
#define AEW_DISCOVER_WORDS 3
constexpr int align_ws_col(int words) { return 4 * (1 + words); }
// the sweep kernels' prologue: the wave's index in its workgroup (wave-uniform; it picks the wave's ring), its lane and
// its pair.  -> 0: no pair is left for this wave
template <class Rec>
__device__ __forceinline__ int align_wave_of(const Rec& p, int& w, int& lane, int& pi) {
    w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    lane = threadIdx.x & 63;
    pi = blockIdx.x * AEW_ALIGN_WAVES + w;
    return pi < p.n_pairs;
}
// what the sweep reads and writes of one pair (n, m >= 1, every record checked)
struct align_sweep_in {
    const float *A, *B;                                 // element (0, 0) of the two sequences
    int64_t afs, acs, bfs, bcs;
    int n, m, D, metric;
    float* wsC;                                         // the boundary row: m entries each (formed, not followed, where the
    int *wsS, *wsB;                                     // record's ws is NULL); wsB: SUB only
    uint8_t* back;                                      // !SUB: n * m back bytes, or NULL
    float* pc;                                          // SUB: the profile, m entries each
    int *ps, *pb;
};
struct align_sweep_out {
    float C;                                            // what each lane carried last: lane (n - 1) & 63 holds cell (n-1, m-1)
    int S;
    bool bad;                                           // this lane met a local distance that is not finite
};
// the sweep's input as both ops fill it; the caller adds `back`, or wsB and the profile
template <class Rec, class View>
__device__ __forceinline__ align_sweep_in align_sweep_of(const Rec& p, const View& v, int pi, int64_t wstride) {
    align_sweep_in q = {};
    q.A = (const float*)p.feat_a + v.sa.base;
    q.B = (const float*)p.feat_b + v.sb.base;
    q.afs = v.sa.frame_stride; q.acs = v.sa.chan_stride; q.bfs = v.sb.frame_stride; q.bcs = v.sb.chan_stride;
    q.n = v.sa.len; q.m = v.sb.len; q.D = p.D; q.metric = p.metric;
    q.wsC = (float*)p.ws + (int64_t)pi * wstride;
    q.wsS = (int*)p.ws + ((int64_t)p.n_pairs + pi) * wstride;
    return q;
}
// Phase (A) of a sweep, shared by align_sweep and discover_sweep (aew_discover.hip): the local distances of the columns
// [j0, j0 + 64) that exist, for the lane's row, into its ring.  a: the lane's A row in registers (DR > 0), arow: the same
// row in memory (DR == 0 reads it again for every column).  live(j): does column j of this row count towards the
// verdict.  bad: raised when this lane meets a local distance that is not finite in a cell that counts.
template <int DR, class Live>
__device__ __forceinline__ void align_fill_ring(const align_sweep_in& q, const float* a, const float* arow, const int j0,
                                                const bool row_on, float* ring, const int lane, bool& bad, Live live) {
    const float* B = q.B;
    const int64_t acs = q.acs, bfs = q.bfs, bcs = q.bcs;
    const int m = q.m, D = q.D;
    const bool sq = q.metric == AEW_ALIGN_SQEUCLID;
    const int jn = m - j0 < 64 ? m - j0 : 64;
    if (DR > 0 && jn > 0) {
        // lane l fetches frame j0 + l (the last frame again behind m); column jj's frame is then lane jj's registers,
        // handed to the whole wave by a uniform-index lane read: no memory access inside the column loop
        float b[DR > 0 ? DR : 1];
        const float* bl = B + (int64_t)(j0 + lane < m ? j0 + lane : m - 1) * bfs;
#pragma unroll
        for (int k = 0; k < DR; ++k) b[k] = k < D ? bl[k * bcs] : 0.f;
        for (int jj = 0; jj < jn; ++jj) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < DR; ++k) {
                const float t = a[k] - align_lane(b[k], jj);
                acc = acc + t * t;
            }
            const float d = sq ? acc : sqrtf(acc);                               // sqrtf is IEEE-rounded here
            bad |= row_on && live(j0 + jj) && !isfinite(d);
            ring[((j0 + jj) & (AEW_ALIGN_RING - 1)) * 64 + lane] = d;
        }
    }
    for (int jj = 0; DR == 0 && jj < jn; ++jj) {
        const float* brow = B + (int64_t)(j0 + jj) * bfs;
        float acc = 0.f;
        for (int k = 0; k < D; ++k) {
            const float t = arow[k * acs] - brow[k * bcs];
            acc = acc + t * t;
        }
        const float d = sq ? acc : sqrtf(acc);
        bad |= row_on && live(j0 + jj) && !isfinite(d);
        ring[((j0 + jj) & (AEW_ALIGN_RING - 1)) * 64 + lane] = d;
    }
}

// DR > 0: D <= DR, the lane's A row in DR registers (zeros behind D: t = 0 - 0, acc + 0 * 0 = acc, the same bits).
// DR == 0: any D, the A row is read again for every column.
// SUB: subsequence DTW.  Row 0 has no left predecessor - every column starts a match - so the start column (B, O beside
// C, S) travels with every carried value, through a third boundary row; the lane that owns row n - 1 stores the three
// profile entries of each column; there is no back byte.  Without SUB none of that exists.
template <int DR, bool SUB>
__device__ __forceinline__ align_sweep_out align_sweep(const align_sweep_in& q, float* ring, const int lane) {
    const float* A = q.A;
    const int64_t afs = q.afs, acs = q.acs;
    const int n = q.n, m = q.m, D = q.D;
    const int nchunk = (m + 63 + 63) >> 6;                                       // sweep steps t = 0 .. m + 62
    bool bad = false;
    float cL = 0.f;
    int sL = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool row_on = i < n;
        const float* arow = A + (int64_t)(row_on ? i : n - 1) * afs;             // (idle lanes repeat the last row: reads stay inside)
        float a[DR > 0 ? DR : 1];
        if (DR > 0) {
#pragma unroll
            for (int k = 0; k < DR; ++k) a[k] = k < D ? arow[k * acs] : 0.f;
        }
        const bool keep_bottom = i0 + 64 < n;                                    // a strip follows: its top row is this one's bottom
        const bool last_row = i == n - 1;                                        // (SUB) this lane's cells are the profile
        float upPrevC = 0.f, topC = 0.f;
        int upPrevS = 0, topS = 0, upPrevB = 0, topB = 0, bL = 0;
        cL = 0.f; sL = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int j0 = c << 6;
            // (A) local distances of the columns [j0, j0 + 64) that exist
            align_fill_ring<DR>(q, a, arow, j0, row_on, ring, lane, bad, [](int) { return true; });
            // the top row's columns [j0, j0 + 64): lane l holds column j0 + l
            if (i0 > 0 && j0 + lane < m) {
                topC = q.wsC[j0 + lane]; topS = q.wsS[j0 + lane];
                if constexpr (SUB) topB = q.wsB[j0 + lane];
            }
            // (B) sweep steps t = j0 .. j0 + 63
            float dnext = ring[((j0 - lane) & (AEW_ALIGN_RING - 1)) * 64 + lane];
            for (int tt = 0; tt < 64; ++tt) {
                const int j = j0 + tt - lane;
                float upC = align_up1(cL);
                int upS = align_up1(sL), upB = 0;
                if constexpr (SUB) upB = align_up1(bL);
                const float tC = align_lane(topC, tt);
                const int tS = align_lane(topS, tt);
                if (lane == 0) { upC = tC; upS = tS; }
                if constexpr (SUB) {
                    const int tB = align_lane(topB, tt);
                    if (lane == 0) upB = tB;
                }
                const float d = dnext;
                dnext = ring[((j + 1) & (AEW_ALIGN_RING - 1)) * 64 + lane];      // (the next step's, fetched under this one)
                // selects, not branches: the lanes of a step differ in which predecessors exist.  The terms in SUB state at
                // compile time what SUB implies - has_left only under has_up; row 0, all origins, uses none of b1 .. o2 -
                // and keep the serial chain of each mode as short as it was alone: one more scalar op per step costs ~1 %.
                const bool on = row_on && j >= 0 && j < m;
                const bool has_up = i > 0, has_left = SUB ? (has_up && j > 0) : (j > 0);
                const bool take_up = (SUB || has_up) && (!has_left || upC < upPrevC);    // (i-1, j) beats (i-1, j-1), or that one is missing
                const float b1 = take_up ? upC : upPrevC;
                const int s1 = take_up ? upS : upPrevS;
                const int o1 = take_up ? upB : upPrevB;                          // (the start column: zeros without SUB, and unused)
                const bool take_left = has_left && ((!SUB && !has_up) || cL < b1);       // (i, j-1) beats the better of the two
                const float b2 = take_left ? cL : b1;
                const int s2 = take_left ? sL : s1;
                const int o2 = take_left ? bL : o1;
                const bool origin = !has_up && (SUB || !has_left);               // (SUB: all of row 0)
                const float C = origin ? d : d + b2;
                const int S = origin ? 1 : s2 + 1;
                const int O = origin ? j : o2;
                const int which = take_left ? 2 : (take_up ? 1 : 0);             // (the back byte: unused under SUB)
                if (on) {
                    if constexpr (SUB) {
                        if (last_row) { q.pc[j] = C; q.ps[j] = S; q.pb[j] = O; }
                    } else {
                        if (q.back) q.back[(int64_t)i * m + j] = (uint8_t)which;
                    }
                    if (keep_bottom && lane == 63) {
                        q.wsC[j] = C; q.wsS[j] = S;
                        if constexpr (SUB) q.wsB[j] = O;
                    }
                }
                upPrevC = on ? upC : upPrevC; upPrevS = on ? upS : upPrevS;
                cL = on ? C : cL; sL = on ? S : sL;
                if constexpr (SUB) { upPrevB = on ? upB : upPrevB; bL = on ? O : bL; }
            }
        }
        __threadfence();                                                         // the bottom row's stores, before the next strip loads them
    }
    return {cL, sL, bad};
}

// ---- DTW ---------------------------------------------------------------------------------------------------------------
template <int DR>
__global__ __launch_bounds__(64 * AEW_ALIGN_WAVES) void k_align_dtw(const aew_seq_align_t p, const int64_t wstride) {
    __shared__ float ring_all[AEW_ALIGN_WAVES][AEW_ALIGN_RING * 64];
    int w, lane, pi;
    if (!align_wave_of(p, w, lane, pi)) return;                                  // wave-uniform, like every return below
    const align_pair_view v = align_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len;
    if (n == 0 || m == 0) {
        if (lane == 0) { p.cost[pi] = INFINITY; p.steps[pi] = 0; }
        return;
    }
    align_sweep_in q = align_sweep_of(p, v, pi, wstride);
    q.back = p.back ? p.back + v.pr.back_base : nullptr;
    const align_sweep_out r = align_sweep<DR, false>(q, ring_all[w], lane);
    const float outC = __shfl(r.C, (n - 1) & 63, 64);
    const int outS = __shfl(r.S, (n - 1) & 63, 64);
    const bool any_bad = __any(r.bad ? 1 : 0) != 0;
    if (lane == 0) {
        p.cost[pi] = any_bad ? NAN : outC;
        p.steps[pi] = any_bad ? 0 : outS;
        if (any_bad) atomicAdd(p.bad, 1u);
    }
}

// one wave per pair: lane 0 walks the back-pointers from (n-1, m-1), all lanes fill what is left of the capacity
__global__ __launch_bounds__(64) void k_align_path(const aew_seq_align_t p, const int64_t wstride) {
    const int pi = blockIdx.x, lane = threadIdx.x;
    const align_pair_view v = align_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len;
    if (n == 0 || m == 0) return;
    const int cap = n + m - 1;
    int st = p.steps[pi];
    if (st < 0 || st > cap) st = 0;
    int32_t* out = p.path + 2 * v.pr.path_base;
    for (int e = st + lane; e < cap; e += 64) { out[2 * e] = -1; out[2 * e + 1] = -1; }
    if (lane != 0) return;
    const uint8_t* back = p.back + v.pr.back_base;
    int i = n - 1, j = m - 1;
    for (int e = st - 1; e >= 0; --e) {
        out[2 * e] = i; out[2 * e + 1] = j;
        const int which = back[(int64_t)i * m + j];
        if (which != 2) --i;
        if (which != 1) --j;
        if (i < 0) i = 0;                                                        // (bytes that are no path: stay inside the matrix)
        if (j < 0) j = 0;
    }
}

// ---- EDIT --------------------------------------------------------------------------------------------------------------
// The same sweep over the integer recurrence with its virtual borders E(-1, j) = j + 1, E(i, -1) = i + 1, E(-1, -1) = 0.
// Lane 0 takes symbol b[t] at step t, every other lane the symbol the lane below held a step earlier.
__global__ __launch_bounds__(64 * AEW_ALIGN_EDIT_WAVES) void k_align_edit(const aew_seq_align_t p, const int64_t wstride) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * AEW_ALIGN_EDIT_WAVES + w;
    if (pi >= p.n_pairs) return;
    const align_pair_view v = align_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len;
    if (n == 0 || m == 0) {
        if (lane == 0) { p.cost[pi] = (float)(n + m); p.steps[pi] = n + m; }
        return;
    }
    const int64_t* A = (const int64_t*)p.feat_a + v.sa.base;
    const int64_t* B = (const int64_t*)p.feat_b + v.sb.base;
    const int64_t afs = v.sa.frame_stride, bfs = v.sb.frame_stride;
    int* wsE = (int*)p.ws + (int64_t)pi * wstride;
    const int nchunk = (m + 63 + 63) >> 6;
    int left = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool row_on = i < n;
        const int64_t asym = A[(int64_t)(row_on ? i : n - 1) * afs];
        const bool keep_bottom = i0 + 64 < n;
        int diag = i;                                                            // E(i-1, -1)
        left = i + 1;                                                            // E(i, -1)
        int topE = 0;
        int64_t bsym = 0, bnext = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int j0 = c << 6, jt = j0 + lane;
            bnext = jt < m ? B[(int64_t)jt * bfs] : 0;
            topE = i0 > 0 ? (jt < m ? wsE[jt] : 0) : jt + 1;
            for (int tt = 0; tt < 64; ++tt) {
                const int j = j0 + tt - lane;
                int up = align_up1(left);
                int64_t bs = align_up1(bsym);
                const int tE = align_lane(topE, tt);
                const int64_t tb = align_lane(bnext, tt);
                if (lane == 0) { up = tE; bs = tb; }
                bsym = bs;
                if (row_on && j >= 0 && j < m) {
                    int e = diag + (asym != bsym ? 1 : 0);
                    e = up + 1 < e ? up + 1 : e;
                    e = left + 1 < e ? left + 1 : e;
                    if (keep_bottom && lane == 63) wsE[j] = e;
                    diag = up;
                    left = e;
                }
            }
        }
        __threadfence();
    }
    const int outE = __shfl(left, (n - 1) & 63, 64);
    if (lane == 0) { p.cost[pi] = (float)outE; p.steps[pi] = outE; }
}

// ---- the launchers' shared parts (launch_seq_search, aew_search.hip, is the other caller) ------------------------------
// The host checks of what aew_seq_align_t and aew_seq_search_t have in common, in the order that fixes which code a
// record with several defects gets: the fields (AEW_E_ARG) - own_ok is the verdict on the op's own ones -, the pointers'
// alignment (AEW_E_ALIGN; own_ptrs: the op's own 4-byte pointers or-ed together), then every record of the host tables
// (AEW_E_ARG), with room(pair, n, m) the op's own check of a pair.  frames: fp32 frames under a metric, else int64
// symbols.  ws_col: workspace bytes per pair and column (align_ws_col).  -> 0 and *wstride_out, the longest B side among
// the pairs that need boundary rows.
template <class Rec, class Room>
static int align_check_record(const Rec& p, bool frames, bool own_ok, uintptr_t own_ptrs, int ws_col, Room room, int64_t* wstride_out) {
    if (frames && p.metric != AEW_ALIGN_EUCLID && p.metric != AEW_ALIGN_SQEUCLID) return AEW_E_ARG;
    if (p.D < 1 || p.D > AEW_ALIGN_MAX_D) return AEW_E_ARG;
    if (p.n_pairs < 1 || p.n_pairs > (1 << 24) || p.n_a < 1 || p.n_b < 1) return AEW_E_ARG;
    if (!p.seq_a || !p.seq_a_host || !p.seq_b || !p.seq_b_host || !p.pairs || !p.pairs_host) return AEW_E_ARG;
    const int64_t fmax = (int64_t)1 << 50;
    if (p.n_feat_a < 0 || p.n_feat_a > fmax || p.n_feat_b < 0 || p.n_feat_b > fmax) return AEW_E_ARG;
    if ((p.n_feat_a > 0 && !p.feat_a) || (p.n_feat_b > 0 && !p.feat_b)) return AEW_E_ARG;
    if (p.ws_bytes < 0 || !own_ok) return AEW_E_ARG;
    if (((uintptr_t)p.seq_a | (uintptr_t)p.seq_a_host | (uintptr_t)p.seq_b | (uintptr_t)p.seq_b_host | (uintptr_t)p.pairs |
         (uintptr_t)p.pairs_host) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.feat_a | (uintptr_t)p.feat_b) & (frames ? 3 : 7)) return AEW_E_ALIGN;
    if (((uintptr_t)p.ws | own_ptrs) & 3) return AEW_E_ALIGN;
    for (int i = 0; i < p.n_a; ++i)
        if (!align_seq_ok(p.seq_a_host[i], p.D, p.n_feat_a)) return AEW_E_ARG;
    for (int i = 0; i < p.n_b; ++i)
        if (!align_seq_ok(p.seq_b_host[i], p.D, p.n_feat_b)) return AEW_E_ARG;
    int64_t wstride = 0;
    for (int i = 0; i < p.n_pairs; ++i) {
        const auto& pr = p.pairs_host[i];
        if (!align_pair_ok(pr.a, pr.b, p.n_a, p.n_b)) return AEW_E_ARG;
        const int n = p.seq_a_host[pr.a].len, m = p.seq_b_host[pr.b].len;
        if (!room(pr, n, m)) return AEW_E_ARG;
        if (n > 64 && m > wstride) wstride = m;
    }
    if (wstride > 0 && (!p.ws || p.ws_bytes / ws_col / p.n_pairs < wstride)) return AEW_E_ARG;
    *wstride_out = wstride;
    return 0;
}

// D -> DR, the one ladder: f(std::integral_constant<int, DR>) with the least DR >= D of 4 .. 64, or 0 (any D)
template <class F>
static void align_dispatch_D(int D, F f) {
    if (D <= 4) f(std::integral_constant<int, 4>());
    else if (D <= 8) f(std::integral_constant<int, 8>());
    else if (D <= 12) f(std::integral_constant<int, 12>());
    else if (D <= 16) f(std::integral_constant<int, 16>());
    else if (D <= 32) f(std::integral_constant<int, 32>());
    else if (D <= 64) f(std::integral_constant<int, 64>());
    else f(std::integral_constant<int, 0>());
}

// A sweep and the kernel behind it on the same stream - the path, or a pick; NULL: none -, one wave per pair each.
// sweep_of(dr) -> the sweep kernel whose DR is decltype(dr)::value.  The second kernel is not launched behind an error.
template <class Rec, class SweepOf>
static int align_launch_sweep(const Rec& p, int64_t wstride, hipStream_t st, SweepOf sweep_of, void (*behind)(Rec, int64_t)) {
    const unsigned g = (unsigned)((p.n_pairs + AEW_ALIGN_WAVES - 1) / AEW_ALIGN_WAVES);
    align_dispatch_D(p.D, [&](auto dr) {
        hipLaunchKernelGGL(sweep_of(dr), dim3(g), dim3(64 * AEW_ALIGN_WAVES), 0, st, p, wstride);
    });
    const int rc = (int)hipGetLastError();
    if (rc || !behind) return rc;
    hipLaunchKernelGGL(behind, dim3((unsigned)p.n_pairs), dim3(64), 0, st, p, wstride);
    return (int)hipGetLastError();
}

// ---- the launcher ------------------------------------------------------------------------------------------------------
static int launch_seq_align(const aew_seq_align_t& p, hipStream_t st) {
    const bool edit = p.mode == AEW_ALIGN_EDIT;
    const bool own_ok = (p.mode == AEW_ALIGN_DTW || edit) && !(edit && p.D != 1) && p.cost && p.steps && p.bad &&
                        !(p.path && !p.back) && !(edit && (p.back || p.path)) && !(p.back && p.n_back < 0) && !(p.path && p.n_path < 0);
    const uintptr_t own_ptrs = (uintptr_t)p.cost | (uintptr_t)p.steps | (uintptr_t)p.bad | (uintptr_t)p.path;
    int64_t wstride = 0;
    const int bad = align_check_record(p, !edit, own_ok, own_ptrs, align_ws_col(AEW_ALIGN_WORDS), [&](const aew_align_pair_t& pr, int n, int m) {
        return !p.back || align_room_ok(pr, n, m, p.n_back, p.path != nullptr, p.n_path);
    }, &wstride);
    if (bad) return bad;
    if (edit) {
        const unsigned g = (unsigned)((p.n_pairs + AEW_ALIGN_EDIT_WAVES - 1) / AEW_ALIGN_EDIT_WAVES);
        hipLaunchKernelGGL(k_align_edit, dim3(g), dim3(64 * AEW_ALIGN_EDIT_WAVES), 0, st, p, wstride);
        return (int)hipGetLastError();
    }
    return align_launch_sweep(p, wstride, st, [](auto dr) { return k_align_dtw<decltype(dr)::value>; }, p.path ? k_align_path : nullptr);
}
