// aew_search.hip — AEW_OP_SEQ_SEARCH: subsequence dynamic time warping of a query against a document, the match free to
// start and end at any document frame, and the n_hits best non-overlapping matches of every pair; one WAVEFRONT per pair
// (aewavenet.h states the rule and the records' checks).
//
// Shape.  k_search_sweep calls the sweep k_align_dtw calls - align_sweep<DR, SUB> in aew_align.hip: strips of 64 query
// rows, lane r owns row i0 + r, the local distances of 64 columns in a per-lane ring in LDS, the anti-diagonals walked
// with one DPP move per carried value, the strip's bottom row through the workspace - with SUB = true: row 0 has no left
// predecessor - every column starts a match - so the start column B travels with C and S; the lane that owns row n - 1
// stores the three profile entries of each column; there is no back matrix.  The kernel itself only loads and checks its
// pair, fills the sweep's input and leaves its verdict on the pair in count[p] (0, or -1: a local distance was not
// finite) for the pick, which then owns every output of the pair; the launcher shares its record checks, its D ladder
// and its two launches with launch_seq_align.  k_search_pick, a second launch behind the first on the same stream, runs
// n_hits rounds of a masked arg-min over the pair's profile; the intervals chosen so far live in registers (lane q holds
// hit q), so there is no mask array.  That body is seq_pick, here, under the policy search_pick; k_discover_pick
// (aew_discover.hip) runs it under its own.
//
// Nothing here waits on another wave: no __syncthreads, no flag, no atomic but the count of pairs that are not finite.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_segment.hip).
#pragma once
#include "aew_align.hip"

// ---- the records' checks, ONE definition for the launcher (host copies) and the kernels (device copies) ---------------
// 1 if the pair's m profile entries lie inside [0, n_prof)
__host__ __device__ __forceinline__ int search_room_ok(const aew_search_pair_t& p, int m, int64_t n_prof) {
    return p.prof_base >= 0 && m <= n_prof && p.prof_base <= n_prof - m;
}

typedef seq_pair_view<aew_search_pair_t> search_pair_view;
__device__ __forceinline__ search_pair_view search_load_pair(const aew_seq_search_t& p, int pi, int64_t wstride) {
    search_pair_view v = seq_load_pair(p, pi, wstride);
    if (v.ok && !search_room_ok(v.pr, v.sb.len, p.n_prof)) v.ok = 0;
    return v;
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------
// DR as in k_align_dtw: D <= DR with the lane's query row in DR registers, or 0 for any D.
template <int DR>
__global__ __launch_bounds__(64 * AEW_ALIGN_WAVES) void k_search_sweep(const aew_seq_search_t p, const int64_t wstride) {
    __shared__ float ring_all[AEW_ALIGN_WAVES][AEW_ALIGN_RING * 64];
    int w, lane, pi;
    if (!align_wave_of(p, w, lane, pi)) return;                                  // wave-uniform, like every return below
    const search_pair_view v = search_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int n = v.sa.len, m = v.sb.len;
    if (n == 0 || m == 0) return;                                                // (the pick writes what an empty pair gets)
    align_sweep_in q = align_sweep_of(p, v, pi, wstride);
    q.wsB = (int*)p.ws + (2 * (int64_t)p.n_pairs + pi) * wstride;
    q.pc = p.prof_cost + v.pr.prof_base;
    q.ps = p.prof_steps + v.pr.prof_base;
    q.pb = p.prof_start + v.pr.prof_base;
    const align_sweep_out r = align_sweep<DR, true>(q, ring_all[w], lane);
    const bool any_bad = __any(r.bad ? 1 : 0) != 0;
    if (lane == 0) p.count[pi] = any_bad ? -1 : 0;                               // the verdict, for the pick
}

// ---- the pick ----------------------------------------------------------------------------------------------------------
// The pick of search and discover (aew_discover.hip), one wave per pair: the n_hits best entries of the pair's profile
// whose intervals do not overlap, best first.  Lane l scans the entries l, l + 64, ..; hit q's interval sits in lane q's
// registers, so there is no mask array.  empty: a side of the pair has no frame; *count: the sweep's verdict on the way
// in (not 0: the pair is hurt, it was not finite), the number of hits on the way out.  A Pick gives
//   len                                  the entries of the profile,
//   candidate(x, key, start) -> ok       entry x: may it be a hit, its key, where its interval [start, x] begins,
//   better(a, b)                         does key a beat key b (strict; equal keys: the least entry wins),
//   fill(x, hurt)                        the profile entry of an empty or hurt pair,
//   hit(r, x, store) -> start            hit r is entry x: its start and, under `store`, its slot,
//   pad(r)                               slot r behind the hits that exist.
template <class Pick>
__device__ __forceinline__ void seq_pick(const Pick& pk, const int H, const bool empty, int* count, uint32_t* bad, const int lane) {
    const bool hurt = !empty && *count != 0;
    int found = 0;
    if (empty || hurt) {
        for (int x = lane; x < pk.len; x += 64) pk.fill(x, hurt);
        if (hurt && lane == 0) atomicAdd(bad, 1u);
    } else {
        int ivs = 0, ive = 0;
        for (int r = 0; r < H; ++r) {
            float bk = 0.f;
            int bx = INT_MAX;                                                    // no entry yet
            for (int x = lane; x < pk.len; x += 64) {
                float key;
                int start;
                bool ok = pk.candidate(x, key, start);
                for (int q = 0; q < r; ++q) ok = ok && !(start <= align_lane(ive, q) && x >= align_lane(ivs, q));
                if (ok && (bx == INT_MAX || pk.better(key, bk))) { bk = key; bx = x; }   // (x ascends: a strict test keeps the least x)
            }
            for (int off = 32; off > 0; off >>= 1) {
                const float ok_ = __shfl_xor(bk, off, 64);
                const int ox = __shfl_xor(bx, off, 64);
                if (ox != INT_MAX && (bx == INT_MAX || pk.better(ok_, bk) || (ok_ == bk && ox < bx))) { bk = ok_; bx = ox; }
            }
            if (bx == INT_MAX) break;                                            // (wave-uniform: every lane holds the same entry)
            const int start = pk.hit(r, bx, lane == 0);
            if (lane == r) { ivs = start; ive = bx; }
            ++found;
        }
    }
    for (int r = found + lane; r < H; r += 64) pk.pad(r);
    if (lane == 0) *count = found;
}

// search: the entries are the document frames a match ENDS at, the key its cost or mean cost, the least wins
struct search_pick {
    float* pc;                                          // the pair's profile
    int *ps, *pb;
    int* hits;                                          // the pair's n_hits slots
    float* hcost;
    int* hsteps;
    int len, min_len, max_len;
    bool by_mean;
    __device__ __forceinline__ bool candidate(int j, float& key, int& start) const {
        const float c = pc[j];
        const int b = pb[j];
        key = by_mean ? c / (float)ps[j] : c;                                    // the division is IEEE-rounded here
        const int len = j - b + 1;
        start = b;
        return isfinite(key) && len >= min_len && (max_len <= 0 || len <= max_len);
    }
    __device__ __forceinline__ static bool better(float a, float b) { return a < b; }
    __device__ __forceinline__ void fill(int j, bool hurt) const { pc[j] = hurt ? NAN : INFINITY; ps[j] = 0; pb[j] = -1; }
    __device__ __forceinline__ int hit(int r, int j, bool store) const {
        const int start = pb[j];
        if (store) { hits[2 * r] = start; hits[2 * r + 1] = j; hcost[r] = pc[j]; hsteps[r] = ps[j]; }
        return start;
    }
    __device__ __forceinline__ void pad(int r) const { hits[2 * r] = -1; hits[2 * r + 1] = -1; hcost[r] = INFINITY; hsteps[r] = 0; }
};
__global__ __launch_bounds__(64) void k_search_pick(const aew_seq_search_t p, const int64_t wstride) {
    const int pi = blockIdx.x, lane = threadIdx.x;
    const search_pair_view v = search_load_pair(p, pi, wstride);
    if (!v.ok) return;
    const int64_t lo = v.pr.prof_base, slot = (int64_t)pi * p.n_hits;
    const search_pick pk = {p.prof_cost + lo, p.prof_steps + lo, p.prof_start + lo, p.hits + 2 * slot, p.hit_cost + slot,
                            p.hit_steps + slot, v.sb.len, p.min_len, p.max_len, p.rank == AEW_SEARCH_MEAN};
    seq_pick(pk, p.n_hits, v.sa.len == 0 || v.sb.len == 0, p.count + pi, p.bad, lane);
}

// ---- the launcher ------------------------------------------------------------------------------------------------------
static int launch_seq_search(const aew_seq_search_t& p, hipStream_t st) {
    const bool own_ok = (p.rank == AEW_SEARCH_MEAN || p.rank == AEW_SEARCH_COST) && p.n_hits >= 1 && p.n_hits <= AEW_SEARCH_MAX_HITS &&
                        p.min_len >= 0 && p.max_len >= 0 && p.prof_cost && p.prof_steps && p.prof_start && p.hits && p.hit_cost &&
                        p.hit_steps && p.count && p.bad && p.n_prof >= 0;
    const uintptr_t own_ptrs = (uintptr_t)p.prof_cost | (uintptr_t)p.prof_steps | (uintptr_t)p.prof_start | (uintptr_t)p.hits |
                               (uintptr_t)p.hit_cost | (uintptr_t)p.hit_steps | (uintptr_t)p.count | (uintptr_t)p.bad;
    int64_t wstride = 0;
    const int bad = align_check_record(p, true, own_ok, own_ptrs, align_ws_col(AEW_SEARCH_WORDS), [&](const aew_search_pair_t& pr, int, int m) {
        return search_room_ok(pr, m, p.n_prof);
    }, &wstride);
    if (bad) return bad;
    return align_launch_sweep(p, wstride, st, [](auto dr) { return k_search_sweep<decltype(dr)::value>; }, k_search_pick);
}
