// aew_search.hip — AEW_OP_SEQ_SEARCH: subsequence dynamic time warping of a query against a document, the match free to
// start and end at any document frame, and the n_hits best non-overlapping matches of every pair; one WAVEFRONT per pair
// (aewavenet.h states the rule and the records' checks).
//
// Shape.  k_search_sweep is k_align_dtw's sweep (aew_align.hip: strips of 64 query rows, lane r owns row i0 + r, the
// local distances of 64 columns in a per-lane ring in LDS, the anti-diagonals walked with one DPP move per carried value,
// the strip's bottom row through the workspace) with three differences: row 0 has no left predecessor - every column
// starts a match - so the start column B travels with C and S; the lane that owns row n - 1 stores the three profile
// entries of each column; there is no back matrix.  k_search_pick, a second launch behind the first on the same stream,
// runs n_hits rounds of a masked arg-min over the pair's profile; the intervals chosen so far live in registers (lane q
// holds hit q), so there is no mask array.  The sweep leaves its verdict on the pair in count[p] (0, or -1: a local
// distance was not finite) for the pick, which then owns every output of the pair.
//
// Nothing here waits on another wave: no __syncthreads, no flag, no atomic but the count of pairs that are not finite.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_segment.hip).
#pragma once
#include "aew_align.hip"

// ---- the records' checks, ONE definition for the launcher (host copies) and the kernels (device copies) ---------------
__host__ __device__ __forceinline__ int search_pair_ok(const aew_search_pair_t& p, int n_a, int n_b) {
    return p.a >= 0 && p.a < n_a && p.b >= 0 && p.b < n_b;
}
// 1 if the pair's m profile entries lie inside [0, n_prof)
__host__ __device__ __forceinline__ int search_room_ok(const aew_search_pair_t& p, int m, int64_t n_prof) {
    return p.prof_base >= 0 && m <= n_prof && p.prof_base <= n_prof - m;
}

struct search_pair_view {
    aew_search_pair_t pr;
    aew_align_seq_t sa, sb;
    int ok;
};
__device__ __forceinline__ search_pair_view search_load_pair(const aew_seq_search_t& p, int pi, int64_t wstride) {
    search_pair_view v;
    v.ok = 0;
    v.pr = p.pairs[pi];
    if (!search_pair_ok(v.pr, p.n_a, p.n_b)) return v;
    v.sa = p.seq_a[v.pr.a];
    v.sb = p.seq_b[v.pr.b];
    if (!align_seq_ok(v.sa, p.D, p.n_feat_a) || !align_seq_ok(v.sb, p.D, p.n_feat_b)) return v;
    if (!search_room_ok(v.pr, v.sb.len, p.n_prof)) return v;
    if (v.sa.len > 64 && v.sb.len > 0 && (!p.ws || v.sb.len > wstride)) return v;   // (the tables changed under a captured graph)
    v.ok = 1;
    return v;
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------
// DR as in k_align_dtw: D <= DR with the lane's query row in DR registers, or 0 for any D.
template <int DR>
__global__ __launch_bounds__(64 * AEW_ALIGN_WAVES) void k_search_sweep(const aew_seq_search_t p, const int64_t wstride) {
    __shared__ float ring_all[AEW_ALIGN_WAVES][AEW_ALIGN_RING * 64];
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * AEW_ALIGN_WAVES + w;
    if (pi >= p.n_pairs) return;                                                 // wave-uniform, like every return below
    const search_pair_view v = search_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len, D = p.D;
    if (n == 0 || m == 0) return;                                                // (the pick writes what an empty pair gets)
    float* ring = ring_all[w];
    const float* A = p.feat_a + v.sa.base;
    const float* B = p.feat_b + v.sb.base;
    const int64_t afs = v.sa.frame_stride, acs = v.sa.chan_stride, bfs = v.sb.frame_stride, bcs = v.sb.chan_stride;
    float* wsC = (float*)p.ws + (int64_t)pi * wstride;                           // (formed, not followed, where ws is NULL)
    int* wsS = (int*)p.ws + ((int64_t)p.n_pairs + pi) * wstride;
    int* wsB = (int*)p.ws + (2 * (int64_t)p.n_pairs + pi) * wstride;
    float* pc = p.prof_cost + v.pr.prof_base;
    int* ps = p.prof_steps + v.pr.prof_base;
    int* pb = p.prof_start + v.pr.prof_base;
    const bool sq = p.metric == AEW_ALIGN_SQEUCLID;
    const int nchunk = (m + 63 + 63) >> 6;                                       // sweep steps t = 0 .. m + 62
    bool bad = false;
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
        const bool last_row = i == n - 1;                                        // this lane's cells are the profile
        const bool has_up = i > 0;                                               // row 0: every column starts a match
        float upPrevC = 0.f, topC = 0.f, cL = 0.f;
        int upPrevS = 0, topS = 0, sL = 0, upPrevB = 0, topB = 0, bL = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int j0 = c << 6;
            // (A) local distances of the columns [j0, j0 + 64) that exist
            const int jn = m - j0 < 64 ? m - j0 : 64;
            if (DR > 0 && jn > 0) {
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
                    const float d = sq ? acc : sqrtf(acc);                       // sqrtf is IEEE-rounded here
                    bad |= row_on && !isfinite(d);
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
                bad |= row_on && !isfinite(d);
                ring[((j0 + jj) & (AEW_ALIGN_RING - 1)) * 64 + lane] = d;
            }
            // the top row's columns [j0, j0 + 64): lane l holds column j0 + l
            if (i0 > 0 && j0 + lane < m) { topC = wsC[j0 + lane]; topS = wsS[j0 + lane]; topB = wsB[j0 + lane]; }
            // (B) sweep steps t = j0 .. j0 + 63
            float dnext = ring[((j0 - lane) & (AEW_ALIGN_RING - 1)) * 64 + lane];
            for (int tt = 0; tt < 64; ++tt) {
                const int j = j0 + tt - lane;
                float upC = align_up1(cL);
                int upS = align_up1(sL);
                int upB = align_up1(bL);
                const float tC = align_lane(topC, tt);
                const int tS = align_lane(topS, tt);
                const int tB = align_lane(topB, tt);
                if (lane == 0) { upC = tC; upS = tS; upB = tB; }
                const float d = dnext;
                dnext = ring[((j + 1) & (AEW_ALIGN_RING - 1)) * 64 + lane];      // (the next step's, fetched under this one)
                // selects, not branches: the lanes of a step differ in which predecessors exist
                const bool on = row_on && j >= 0 && j < m;
                const bool has_left = has_up && j > 0;
                const bool take_up = !has_left || upC < upPrevC;                 // (i-1, j) beats (i-1, j-1), or that one is missing
                const float b1 = take_up ? upC : upPrevC;
                const int s1 = take_up ? upS : upPrevS;
                const int o1 = take_up ? upB : upPrevB;
                const bool take_left = has_left && cL < b1;                      // (i, j-1) beats the better of the two
                const float b2 = take_left ? cL : b1;
                const int s2 = take_left ? sL : s1;
                const int o2 = take_left ? bL : o1;
                const float C = has_up ? d + b2 : d;
                const int S = has_up ? s2 + 1 : 1;
                const int O = has_up ? o2 : j;
                if (on) {
                    if (last_row) { pc[j] = C; ps[j] = S; pb[j] = O; }
                    if (keep_bottom && lane == 63) { wsC[j] = C; wsS[j] = S; wsB[j] = O; }
                }
                upPrevC = on ? upC : upPrevC; upPrevS = on ? upS : upPrevS; upPrevB = on ? upB : upPrevB;
                cL = on ? C : cL; sL = on ? S : sL; bL = on ? O : bL;
            }
        }
        __threadfence();                                                         // the bottom row's stores, before the next strip loads them
    }
    const bool any_bad = __any(bad ? 1 : 0) != 0;
    if (lane == 0) p.count[pi] = any_bad ? -1 : 0;                               // the verdict, for the pick
}

// ---- the pick ----------------------------------------------------------------------------------------------------------
// one wave per pair: lane l scans the ends l, l + 64, ..; hit q's interval sits in lane q's registers
__global__ __launch_bounds__(64) void k_search_pick(const aew_seq_search_t p, const int64_t wstride) {
    const int pi = blockIdx.x, lane = threadIdx.x;
    const search_pair_view v = search_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len, H = p.n_hits;
    float* pc = p.prof_cost + v.pr.prof_base;
    int* ps = p.prof_steps + v.pr.prof_base;
    int* pb = p.prof_start + v.pr.prof_base;
    int* hits = p.hits + 2 * (int64_t)pi * H;
    float* hcost = p.hit_cost + (int64_t)pi * H;
    int* hsteps = p.hit_steps + (int64_t)pi * H;
    const bool empty = n == 0 || m == 0;
    const bool hurt = !empty && p.count[pi] != 0;
    int found = 0;
    if (empty || hurt) {
        for (int j = lane; j < m; j += 64) { pc[j] = hurt ? NAN : INFINITY; ps[j] = 0; pb[j] = -1; }
        if (hurt && lane == 0) atomicAdd(p.bad, 1u);
    } else {
        const bool by_mean = p.rank == AEW_SEARCH_MEAN;
        int ivs = 0, ive = 0;
        for (int r = 0; r < H; ++r) {
            float bk = 0.f;
            int bj = INT_MAX;                                                    // no end yet
            for (int j = lane; j < m; j += 64) {
                const float c = pc[j];
                const int b = pb[j];
                const float key = by_mean ? c / (float)ps[j] : c;                // the division is IEEE-rounded here
                const int len = j - b + 1;
                bool ok = isfinite(key) && len >= p.min_len && (p.max_len <= 0 || len <= p.max_len);
                for (int q = 0; q < r; ++q) ok = ok && !(b <= align_lane(ive, q) && j >= align_lane(ivs, q));
                if (ok && (bj == INT_MAX || key < bk)) { bk = key; bj = j; }     // (j ascends: a strict < keeps the least j)
            }
            for (int off = 32; off > 0; off >>= 1) {
                const float ok_ = __shfl_xor(bk, off, 64);
                const int oj = __shfl_xor(bj, off, 64);
                if (oj != INT_MAX && (bj == INT_MAX || ok_ < bk || (ok_ == bk && oj < bj))) { bk = ok_; bj = oj; }
            }
            if (bj == INT_MAX) break;                                            // (wave-uniform: every lane holds the same end)
            const int start = pb[bj];
            if (lane == r) { ivs = start; ive = bj; }
            if (lane == 0) { hits[2 * r] = start; hits[2 * r + 1] = bj; hcost[r] = pc[bj]; hsteps[r] = ps[bj]; }
            ++found;
        }
    }
    for (int r = found + lane; r < H; r += 64) { hits[2 * r] = -1; hits[2 * r + 1] = -1; hcost[r] = INFINITY; hsteps[r] = 0; }
    if (lane == 0) p.count[pi] = found;
}

// ---- the launcher ------------------------------------------------------------------------------------------------------
static int launch_seq_search(const aew_seq_search_t& p, hipStream_t st) {
    if (p.metric != AEW_ALIGN_EUCLID && p.metric != AEW_ALIGN_SQEUCLID) return AEW_E_ARG;
    if (p.rank != AEW_SEARCH_MEAN && p.rank != AEW_SEARCH_COST) return AEW_E_ARG;
    if (p.D < 1 || p.D > AEW_ALIGN_MAX_D) return AEW_E_ARG;
    if (p.n_pairs < 1 || p.n_pairs > (1 << 24) || p.n_a < 1 || p.n_b < 1) return AEW_E_ARG;
    if (p.n_hits < 1 || p.n_hits > AEW_SEARCH_MAX_HITS || p.min_len < 0 || p.max_len < 0) return AEW_E_ARG;
    if (!p.seq_a || !p.seq_a_host || !p.seq_b || !p.seq_b_host || !p.pairs || !p.pairs_host) return AEW_E_ARG;
    if (!p.prof_cost || !p.prof_steps || !p.prof_start || !p.hits || !p.hit_cost || !p.hit_steps || !p.count || !p.bad)
        return AEW_E_ARG;
    const int64_t fmax = (int64_t)1 << 50;
    if (p.n_feat_a < 0 || p.n_feat_a > fmax || p.n_feat_b < 0 || p.n_feat_b > fmax) return AEW_E_ARG;
    if ((p.n_feat_a > 0 && !p.feat_a) || (p.n_feat_b > 0 && !p.feat_b)) return AEW_E_ARG;
    if (p.n_prof < 0 || p.ws_bytes < 0) return AEW_E_ARG;
    if (((uintptr_t)p.seq_a | (uintptr_t)p.seq_a_host | (uintptr_t)p.seq_b | (uintptr_t)p.seq_b_host | (uintptr_t)p.pairs |
         (uintptr_t)p.pairs_host) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.feat_a | (uintptr_t)p.feat_b | (uintptr_t)p.prof_cost | (uintptr_t)p.prof_steps | (uintptr_t)p.prof_start |
         (uintptr_t)p.hits | (uintptr_t)p.hit_cost | (uintptr_t)p.hit_steps | (uintptr_t)p.count | (uintptr_t)p.bad |
         (uintptr_t)p.ws) & 3) return AEW_E_ALIGN;
    for (int i = 0; i < p.n_a; ++i)
        if (!align_seq_ok(p.seq_a_host[i], p.D, p.n_feat_a)) return AEW_E_ARG;
    for (int i = 0; i < p.n_b; ++i)
        if (!align_seq_ok(p.seq_b_host[i], p.D, p.n_feat_b)) return AEW_E_ARG;
    int64_t wstride = 0;                                                         // longest document among the pairs that need boundary rows
    for (int i = 0; i < p.n_pairs; ++i) {
        const aew_search_pair_t& pr = p.pairs_host[i];
        if (!search_pair_ok(pr, p.n_a, p.n_b)) return AEW_E_ARG;
        const int n = p.seq_a_host[pr.a].len, m = p.seq_b_host[pr.b].len;
        if (!search_room_ok(pr, m, p.n_prof)) return AEW_E_ARG;
        if (n > 64 && m > wstride) wstride = m;
    }
    if (wstride > 0 && (!p.ws || p.ws_bytes / 12 / p.n_pairs < wstride)) return AEW_E_ARG;
    const unsigned g = (unsigned)((p.n_pairs + AEW_ALIGN_WAVES - 1) / AEW_ALIGN_WAVES);
    const dim3 blk(64 * AEW_ALIGN_WAVES);
    if (p.D <= 4) hipLaunchKernelGGL(k_search_sweep<4>, dim3(g), blk, 0, st, p, wstride);
    else if (p.D <= 8) hipLaunchKernelGGL(k_search_sweep<8>, dim3(g), blk, 0, st, p, wstride);
    else if (p.D <= 12) hipLaunchKernelGGL(k_search_sweep<12>, dim3(g), blk, 0, st, p, wstride);
    else if (p.D <= 16) hipLaunchKernelGGL(k_search_sweep<16>, dim3(g), blk, 0, st, p, wstride);
    else if (p.D <= 32) hipLaunchKernelGGL(k_search_sweep<32>, dim3(g), blk, 0, st, p, wstride);
    else if (p.D <= 64) hipLaunchKernelGGL(k_search_sweep<64>, dim3(g), blk, 0, st, p, wstride);
    else hipLaunchKernelGGL(k_search_sweep<0>, dim3(g), blk, 0, st, p, wstride);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(k_search_pick, dim3((unsigned)p.n_pairs), dim3(64), 0, st, p, wstride);
    return (int)hipGetLastError();
}
