// aew_discover.hip — AEW_OP_SEQ_DISCOVER: local-alignment dynamic time warping (segmental DTW) of two utterances, the
// alignment free to start and end at any cell, and the n_hits best alignments of every pair whose A ranges do not
// overlap; one WAVEFRONT per pair (aewavenet.h states the rule and the records' checks).
//
// Shape.  discover_sweep<DR> is the sibling of align_sweep<DR, SUB> (aew_align.hip) and keeps its frame: strips of 64 A
// rows, lane r owns row i0 + r, phase (A) - the local distances of 64 columns into the per-lane ring in LDS - is the ONE
// function both call (align_fill_ring), phase (B) walks the anti-diagonals with one DPP move per carried value, the
// strip's bottom row goes through the workspace.  What differs is the recurrence, so (B) is its own: a cell MAXIMISES the
// score H over the predecessors that are alive (H > 0), adds the gain threshold - d and dies (H = 0) where the sum is not
// positive or the cell lies outside the pair's band; with H travel the steps S and the origin (row, column), four words
// per carried value and four boundary rows.  A predecessor that does not exist reads as H = 0 - the registers start at 0,
// the first strip has an all-zero top row - so "exists and is alive" is the one test H > 0 and the lanes of a step need
// no has_up / has_left.  Each lane keeps the running maximum of its row (E, its column, origin, steps) in registers and
// stores the five profile words when its strip ends: no cross-lane reduction.  The kernel leaves its verdict on the pair
// in count[p] (0, or -1: a local distance inside the band was not finite) for the pick, which then owns every output of
// the pair.  k_discover_pick, a second launch behind the first on the same stream, is k_search_pick's body (seq_pick,
// aew_search.hip) over ROWS: n_hits rounds of a masked arg-max, the A ranges chosen so far in registers (lane q holds
// hit q).  The launcher shares its record checks, its pair loader, its D ladder and its two launches with
// launch_seq_align / launch_seq_search.
//
// Nothing here waits on another wave: no __syncthreads, no flag, no atomic but the count of pairs that are not finite.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_search.hip).
#pragma once
#include "aew_search.hip"

// ---- the records' checks, ONE definition for the launcher (host copies) and the kernels (device copies) ---------------
// 1 if the pair's band is one and its n profile entries lie inside [0, n_prof)
__host__ __device__ __forceinline__ int discover_room_ok(const aew_discover_pair_t& p, int n, int64_t n_prof) {
    return p.band >= 0 && p.prof_base >= 0 && n <= n_prof && p.prof_base <= n_prof - n;
}

typedef seq_pair_view<aew_discover_pair_t> discover_pair_view;
__device__ __forceinline__ discover_pair_view discover_load_pair(const aew_seq_discover_t& p, int pi, int64_t wstride) {
    discover_pair_view v = seq_load_pair(p, pi, wstride);
    if (v.ok && !discover_room_ok(v.pr, v.sa.len, p.n_prof)) v.ok = 0;
    return v;
}

// the pair's profile as the pick reads it, n entries each
struct discover_prof {
    float* pe;
    int *pj, *pr, *pc, *ps;
};
__device__ __forceinline__ discover_prof discover_prof_of(const aew_seq_discover_t& p, int64_t lo) {
    return {p.prof_score + lo, p.prof_end + lo, p.prof_row + lo, p.prof_col + lo, p.prof_steps + lo};
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------
// what the sweep reads and writes of one pair beside align_sweep_in (of which it uses the two sequences and wsC / wsS)
struct discover_io {
    int *wsR, *wsO;                                     // the boundary row's origin row and origin column, m entries each
    float* pe;                                          // the profile, n entries each
    int *pj, *pr, *pc, *ps;
    float theta;
    int band;
};
// DR as in align_sweep.  -> this lane met a local distance inside the band that is not finite
template <int DR>
__device__ __forceinline__ bool discover_sweep(const align_sweep_in& q, const discover_io& io, float* ring, const int lane) {
    const float* A = q.A;
    const int64_t afs = q.afs, acs = q.acs;
    const int n = q.n, m = q.m, D = q.D;
    const float theta = io.theta;
    const int lo = io.band > 0 ? io.band : INT_MIN;                              // a cell is inside the band iff j - i >= lo
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
        // the carried cell (i, j-1), the diagonal one (i-1, j-1), the top row; zeros: nothing there, or nothing alive
        float hL = 0.f, upPrevH = 0.f, topH = 0.f;
        int sL = 0, rL = 0, oL = 0, upPrevS = 0, upPrevR = 0, upPrevO = 0, topS = 0, topR = 0, topO = 0;
        float eH = 0.f;                                                          // the row's running maximum and whose it is
        int eJ = -1, eR = -1, eO = -1, eS = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int j0 = c << 6;
            // (A) local distances of the columns [j0, j0 + 64) that exist
            align_fill_ring<DR>(q, a, arow, j0, row_on, ring, lane, bad, [=](int j) { return j - i >= lo; });
            // the top row's columns [j0, j0 + 64): lane l holds column j0 + l (the first strip's stays all zero)
            if (i0 > 0 && j0 + lane < m) {
                topH = q.wsC[j0 + lane]; topS = q.wsS[j0 + lane]; topR = io.wsR[j0 + lane]; topO = io.wsO[j0 + lane];
            }
            // (B) sweep steps t = j0 .. j0 + 63
            float dnext = ring[((j0 - lane) & (AEW_ALIGN_RING - 1)) * 64 + lane];
            for (int tt = 0; tt < 64; ++tt) {
                const int j = j0 + tt - lane;
                float upH = align_up1(hL);
                int upS = align_up1(sL), upR = align_up1(rL), upO = align_up1(oL);
                const float tH = align_lane(topH, tt);
                const int tS = align_lane(topS, tt), tR = align_lane(topR, tt), tO = align_lane(topO, tt);
                if (lane == 0) { upH = tH; upS = tS; upR = tR; upO = tO; }
                const float d = dnext;
                dnext = ring[((j + 1) & (AEW_ALIGN_RING - 1)) * 64 + lane];      // (the next step's, fetched under this one)
                const bool on = row_on && j >= 0 && j < m;
                // selects, not branches.  (i-1, j-1), then (i-1, j), then (i, j-1), each taken only if strictly larger
                const bool take_up = upH > upPrevH;
                const float b1 = take_up ? upH : upPrevH;
                const int s1 = take_up ? upS : upPrevS, r1 = take_up ? upR : upPrevR, o1 = take_up ? upO : upPrevO;
                const bool take_left = hL > b1;
                const float b2 = take_left ? hL : b1;
                const int s2 = take_left ? sL : s1, r2 = take_left ? rL : r1, o2 = take_left ? oL : o1;
                const bool has = b2 > 0.f;                                       // an alive predecessor
                const float g = theta - d;
                const float Hs = has ? b2 + g : g;
                const bool alive = j - i >= lo && Hs > 0.f;                      // (a NaN is not > 0: dead)
                const float H = alive ? Hs : 0.f;
                const int S = alive ? (has ? s2 + 1 : 1) : 0;
                const int R = has ? r2 : i, O = has ? o2 : j;
                if (on && keep_bottom && lane == 63) { q.wsC[j] = H; q.wsS[j] = S; io.wsR[j] = R; io.wsO[j] = O; }
                const bool better = on && H > eH;                                // (j ascends: a strict > keeps the least j)
                eH = better ? H : eH; eJ = better ? j : eJ; eR = better ? R : eR; eO = better ? O : eO; eS = better ? S : eS;
                upPrevH = on ? upH : upPrevH; upPrevS = on ? upS : upPrevS; upPrevR = on ? upR : upPrevR; upPrevO = on ? upO : upPrevO;
                hL = on ? H : hL; sL = on ? S : sL; rL = on ? R : rL; oL = on ? O : oL;
            }
        }
        if (row_on) { io.pe[i] = eH; io.pj[i] = eJ; io.pr[i] = eR; io.pc[i] = eO; io.ps[i] = eS; }
        __threadfence();                                                         // the bottom row's stores, before the next strip loads them
    }
    return bad;
}

template <int DR>
__global__ __launch_bounds__(64 * AEW_ALIGN_WAVES) void k_discover_sweep(const aew_seq_discover_t p, const int64_t wstride) {
    __shared__ float ring_all[AEW_ALIGN_WAVES][AEW_ALIGN_RING * 64];
    int w, lane, pi;
    if (!align_wave_of(p, w, lane, pi)) return;                                  // wave-uniform, like every return below
    const discover_pair_view v = discover_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len;
    if (n == 0 || m == 0) return;                                                // (the pick writes what an empty pair gets)
    const align_sweep_in q = align_sweep_of(p, v, pi, wstride);                  // (wsC / wsS: the boundary row's H and S)
    discover_io io;
    io.wsR = (int*)p.ws + (2 * (int64_t)p.n_pairs + pi) * wstride;
    io.wsO = (int*)p.ws + (3 * (int64_t)p.n_pairs + pi) * wstride;
    io.pe = p.prof_score + v.pr.prof_base;
    io.pj = p.prof_end + v.pr.prof_base;
    io.pr = p.prof_row + v.pr.prof_base;
    io.pc = p.prof_col + v.pr.prof_base;
    io.ps = p.prof_steps + v.pr.prof_base;
    io.theta = p.threshold;
    io.band = v.pr.band;
    const bool bad = discover_sweep<DR>(q, io, ring_all[w], lane);
    const bool any_bad = __any(bad ? 1 : 0) != 0;
    if (lane == 0) p.count[pi] = any_bad ? -1 : 0;                               // the verdict, for the pick
}

// ---- the pick ----------------------------------------------------------------------------------------------------------
// seq_pick (aew_search.hip) over ROWS: the entries are the A rows an alignment ENDS in, the key its score, the largest
// wins; an interval is the hit's A range
struct discover_pick {
    discover_prof prof;
    int* hits;                                          // the pair's n_hits slots
    float* hscore;
    int* hsteps;
    int len, min_len, max_len;
    __device__ __forceinline__ bool candidate(int i, float& key, int& start) const {
        const float e = prof.pe[i];
        const int r0 = prof.pr[i];
        const int la = i - r0 + 1, lb = prof.pj[i] - prof.pc[i] + 1;
        key = e;
        start = r0;
        return e > 0.f && la >= min_len && lb >= min_len && (max_len <= 0 || (la <= max_len && lb <= max_len));
    }
    __device__ __forceinline__ static bool better(float a, float b) { return a > b; }
    __device__ __forceinline__ void fill(int i, bool hurt) const {
        prof.pe[i] = hurt ? NAN : 0.f; prof.pj[i] = -1; prof.pr[i] = -1; prof.pc[i] = -1; prof.ps[i] = 0;
    }
    __device__ __forceinline__ int hit(int r, int i, bool store) const {
        const int start = prof.pr[i];
        if (store) {
            hits[4 * r] = start; hits[4 * r + 1] = i; hits[4 * r + 2] = prof.pc[i]; hits[4 * r + 3] = prof.pj[i];
            hscore[r] = prof.pe[i]; hsteps[r] = prof.ps[i];
        }
        return start;
    }
    __device__ __forceinline__ void pad(int r) const {
        hits[4 * r] = -1; hits[4 * r + 1] = -1; hits[4 * r + 2] = -1; hits[4 * r + 3] = -1;
        hscore[r] = NAN; hsteps[r] = 0;
    }
};
__global__ __launch_bounds__(64) void k_discover_pick(const aew_seq_discover_t p, const int64_t wstride) {
    const int pi = blockIdx.x, lane = threadIdx.x;
    const discover_pair_view v = discover_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int64_t slot = (int64_t)pi * p.n_hits;
    const discover_pick pk = {discover_prof_of(p, v.pr.prof_base), p.hits + 4 * slot, p.hit_score + slot, p.hit_steps + slot,
                              v.sa.len, p.min_len, p.max_len};
    seq_pick(pk, p.n_hits, v.sa.len == 0 || v.sb.len == 0, p.count + pi, p.bad, lane);
}

// ---- the launcher ------------------------------------------------------------------------------------------------------
static int launch_seq_discover(const aew_seq_discover_t& p, hipStream_t st) {
    const bool own_ok = p.n_hits >= 1 && p.n_hits <= AEW_SEARCH_MAX_HITS && p.min_len >= 0 && p.max_len >= 0 &&
                        std::isfinite(p.threshold) && p.prof_score && p.prof_end && p.prof_row && p.prof_col && p.prof_steps &&
                        p.hits && p.hit_score && p.hit_steps && p.count && p.bad && p.n_prof >= 0;
    const uintptr_t own_ptrs = (uintptr_t)p.prof_score | (uintptr_t)p.prof_end | (uintptr_t)p.prof_row | (uintptr_t)p.prof_col |
                               (uintptr_t)p.prof_steps | (uintptr_t)p.hits | (uintptr_t)p.hit_score | (uintptr_t)p.hit_steps |
                               (uintptr_t)p.count | (uintptr_t)p.bad;
    int64_t wstride = 0;
    const int bad = align_check_record(p, true, own_ok, own_ptrs, align_ws_col(AEW_DISCOVER_WORDS), [&](const aew_discover_pair_t& pr, int n, int) {
        return discover_room_ok(pr, n, p.n_prof);
    }, &wstride);
    if (bad) return bad;
    return align_launch_sweep(p, wstride, st, [](auto dr) { return k_discover_sweep<decltype(dr)::value>; }, k_discover_pick);
}
