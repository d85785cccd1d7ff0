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
// finite) for the pick, which then owns every output of the pair; the launcher shares its record checks and its D ladder
// with launch_seq_align.  k_search_pick, a second launch behind the first on the same stream, runs n_hits rounds of a
// masked arg-min over the pair's profile; the intervals chosen so far live in registers (lane q holds hit q), so there
// is no mask array.
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
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * AEW_ALIGN_WAVES + w;
    if (pi >= p.n_pairs) return;                                                 // wave-uniform, like every return below
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
    const bool own_ok = (p.rank == AEW_SEARCH_MEAN || p.rank == AEW_SEARCH_COST) && p.n_hits >= 1 && p.n_hits <= AEW_SEARCH_MAX_HITS &&
                        p.min_len >= 0 && p.max_len >= 0 && p.prof_cost && p.prof_steps && p.prof_start && p.hits && p.hit_cost &&
                        p.hit_steps && p.count && p.bad && p.n_prof >= 0;
    const uintptr_t own_ptrs = (uintptr_t)p.prof_cost | (uintptr_t)p.prof_steps | (uintptr_t)p.prof_start | (uintptr_t)p.hits |
                               (uintptr_t)p.hit_cost | (uintptr_t)p.hit_steps | (uintptr_t)p.count | (uintptr_t)p.bad;
    int64_t wstride = 0;
    const int bad = align_check_record(p, true, own_ok, own_ptrs, 12, [&](const aew_search_pair_t& pr, int, int m) {
        return search_room_ok(pr, m, p.n_prof);
    }, &wstride);
    if (bad) return bad;
    const unsigned g = (unsigned)((p.n_pairs + AEW_ALIGN_WAVES - 1) / AEW_ALIGN_WAVES);
    align_dispatch_D(p.D, [&](auto dr) {
        hipLaunchKernelGGL(k_search_sweep<decltype(dr)::value>, dim3(g), dim3(64 * AEW_ALIGN_WAVES), 0, st, p, wstride);
    });
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(k_search_pick, dim3((unsigned)p.n_pairs), dim3(64), 0, st, p, wstride);
    return (int)hipGetLastError();
}
