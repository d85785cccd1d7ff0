// aew_abx.hip — AEW_OP_ABX_COUNT: the (A, B, X) triples of a labelled item set counted over its N x N distance matrix,
// per X and per group of B items (aewavenet.h states the rule bit for bit and the record's checks).
//
// Shape.  One kernel, one workgroup of ABX_WAVES wavefronts per sorted position x; no workgroup waits for another.
//   gather   the permuted row d(x, .) = D[perm[x] * ld + perm[.]] goes ONCE into LDS, whole: N floats of dynamic LDS
//            and nothing else in LDS (exactly 64 KiB at the largest N, 16384 - the most a launch gets without the
//            per-function opt-in, which this kernel therefore does not need; never staged in pieces, so no N changes
//            the path).  Behind one barrier the row is only read.  X's group comes from a ballot over the group scan.
//   cells    the waves take the groups g = wave, wave + ABX_WAVES, ... in turn.  The record of g, the partner entry and the
//            verdict of abx_cell are wave-uniform.  In a valid cell lane l owns the b's lo + l, lo + l + 64, ... of g; the
//            a's of A's range are read as LDS broadcasts (one address for the wave), four per trip; each pair is
//            abx_w: compares and an integer add in the lane.  x itself lies in A's range only when A's group is X's own;
//            then the lane takes w(d(x, x), d(x, b)) off again instead of testing a != x in the loop.  A shuffle
//            reduction, and lane 0 writes the two words with ordinary stores; an invalid cell gets its two zeros.
// Integer sums: no order changes a bit.  w, the cell's validity and the record's checks are ONE __host__ __device__ /
// host definition each; aew_abx_host runs them on the CPU.
// Part of the library's one translation unit (aewavenet.hip includes it behind aew_search.hip).
#pragma once
#include "aew_common.h"
#include <vector>

#define ABX_WAVES 4                 // wavefronts of a workgroup

// ---- the rule, ONE definition for the kernel and the host twin -----------------------------------------------------------
// twice the error of one triple: X belongs with A, so d(x, a) = p above d(x, b) = q is wrong
__host__ __device__ __forceinline__ uint32_t abx_w(float p, float q) {
    return (p > q ? 1u : 0u) + (p < q ? 0u : 1u);                                 // 2, 0, or 1 for equal / unordered
}
// 1 and A's range [*alo, *ahi) with *self = x lies inside it, if cell (x in group gx, g) is valid; no address is formed
// from a record field that was not range-checked here
__host__ __device__ __forceinline__ int abx_cell(const aew_abx_group_t* groups, const int32_t* partner, int N, int G, int C,
                                                 int S, int mode, int gx, const aew_abx_group_t& gb, int* alo, int* ahi,
                                                 int* self) {
    const aew_abx_group_t rx = groups[gx];
    if ((unsigned)rx.cat >= (unsigned)C || (unsigned)rx.spk >= (unsigned)S) return 0;
    if ((unsigned)gb.cat >= (unsigned)C || (unsigned)gb.spk >= (unsigned)S) return 0;
    if (gb.lo < 0 || gb.hi > N || gb.hi <= gb.lo) return 0;
    if (gb.cat == rx.cat) return 0;
    if (mode == AEW_ABX_WITHIN ? gb.spk != rx.spk : gb.spk == rx.spk) return 0;
    const int pa = partner[(int64_t)rx.cat * S + gb.spk];
    if ((unsigned)pa >= (unsigned)G) return 0;                                    // (-1: no item of X's category under B's speaker)
    const aew_abx_group_t ra = groups[pa];
    if (ra.lo < 0 || ra.hi > N || ra.hi <= ra.lo) return 0;
    *self = pa == gx;
    *alo = ra.lo;
    *ahi = ra.hi;
    return ra.hi - ra.lo - (pa == gx ? 1 : 0) > 0;
}

// ---- the checks of a call, ONE definition for the launcher and the host twin ---------------------------------------------
static int abx_check(const aew_abx_count_t& p, bool host) {
    if (p.mode != AEW_ABX_WITHIN && p.mode != AEW_ABX_ACROSS) return AEW_E_ARG;
    if (p.N < 1 || p.N > AEW_ABX_MAX_N || p.G < 1 || p.G > p.N || p.C < 1 || p.S < 1) return AEW_E_ARG;
    if ((int64_t)p.N * p.G > ((int64_t)1 << 27) || (int64_t)p.C * p.S > (int64_t)p.N * p.G || p.ld < p.N) return AEW_E_ARG;
    if (!p.dist || !p.perm_host || !p.groups_host || !p.partner_host || !p.n || !p.wrong2) return AEW_E_ARG;
    if (!host && (!p.perm || !p.groups || !p.partner)) return AEW_E_ARG;
    if (((uintptr_t)p.dist | (uintptr_t)p.perm | (uintptr_t)p.perm_host | (uintptr_t)p.groups | (uintptr_t)p.groups_host |
         (uintptr_t)p.partner | (uintptr_t)p.partner_host | (uintptr_t)p.n | (uintptr_t)p.wrong2) & 3)
        return AEW_E_ALIGN;
    std::vector<char> seen((size_t)p.N, 0);                                       // host work per launch: N bytes here, one pass
                                                                                  // over perm, the groups and the C * S <= N * G partner words
    for (int x = 0; x < p.N; ++x) {
        const int32_t i = p.perm_host[x];
        if (i < 0 || i >= p.N || seen[i]) return AEW_E_ARG;
        seen[i] = 1;
    }
    int at = 0;
    for (int g = 0; g < p.G; ++g) {
        const aew_abx_group_t& r = p.groups_host[g];
        if (r.lo != at || r.hi <= r.lo || r.hi > p.N) return AEW_E_ARG;
        if (r.cat < 0 || r.cat >= p.C || r.spk < 0 || r.spk >= p.S) return AEW_E_ARG;
        if (p.partner_host[(int64_t)r.cat * p.S + r.spk] != g) return AEW_E_ARG;
        at = r.hi;
    }
    if (at != p.N) return AEW_E_ARG;
    int64_t named = 0;
    for (int64_t k = 0; k < (int64_t)p.C * p.S; ++k) {
        const int32_t v = p.partner_host[k];
        if (v < -1 || v >= p.G) return AEW_E_ARG;
        named += v >= 0;
    }
    return named == p.G ? 0 : AEW_E_ARG;                                          // (with the loop above: exactly the inverse)
}

// ---- the kernel ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ABX_WAVES * 64) void k_abx_count(const aew_abx_count_t p) {
    extern __shared__ __attribute__((aligned(16))) float abx_row[];               // d(x, .): N floats, nothing else (<= 64 KiB)
    const int N = p.N, G = p.G, x = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = p.perm[x];
    const bool row_ok = (unsigned)px < (unsigned)N;
    const float* drow = p.dist + (int64_t)(row_ok ? px : 0) * p.ld;
    for (int j = threadIdx.x; j < N; j += ABX_WAVES * 64) {
        const int pj = p.perm[j];
        abx_row[j] = (row_ok && (unsigned)pj < (unsigned)N) ? drow[pj] : 0.f;
    }
    int gx = -1;                                                                  // X's group: the groups tile [0, N), one holds x.
    for (int g0 = 0; g0 < G && gx < 0; g0 += 64) {                                // Every wave finds it for itself, 64 records a
        const int g = g0 + lane;                                                  // trip, and takes it from the ballot: uniform,
        bool hit = false;                                                         // no LDS word, no second barrier
        if (g < G) {
            const aew_abx_group_t r = p.groups[g];
            hit = r.lo <= x && x < r.hi;
        }
        const uint64_t mask = __ballot(hit ? 1 : 0);
        if (mask) gx = g0 + __ffsll((unsigned long long)mask) - 1;
    }
    if (!row_ok) gx = -1;
    __syncthreads();                                                              // the row, before anybody reads it
    uint32_t* out_n = p.n + (int64_t)x * G;
    uint32_t* out_w = p.wrong2 + (int64_t)x * G;
    for (int g = wave; g < G; g += ABX_WAVES) {
        const aew_abx_group_t gb = p.groups[g];
        int alo = 0, ahi = 0, self = 0;
        const int valid = gx >= 0 && abx_cell(p.groups, p.partner, N, G, p.C, p.S, p.mode, gx, gb, &alo, &ahi, &self);
        if (!valid) {                                                             // wave-uniform
            if (lane == 0) { out_n[g] = 0u; out_w[g] = 0u; }
            continue;
        }
        const float dxx = abx_row[x];
        uint32_t cnt = 0;
        for (int b0 = gb.lo; b0 < gb.hi; b0 += 64) {
            const int b = b0 + lane;
            const bool live = b < gb.hi;
            const float db = abx_row[live ? b : gb.lo];
            uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
            int a = alo;
            for (; a + 4 <= ahi; a += 4) {
                c0 += abx_w(abx_row[a], db);
                c1 += abx_w(abx_row[a + 1], db);
                c2 += abx_w(abx_row[a + 2], db);
                c3 += abx_w(abx_row[a + 3], db);
            }
            for (; a < ahi; ++a) c0 += abx_w(abx_row[a], db);
            uint32_t c = c0 + c1 + c2 + c3;
            if (self) c -= abx_w(dxx, db);
            cnt += live ? c : 0u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) {
            out_n[g] = (uint32_t)(ahi - alo - self) * (uint32_t)(gb.hi - gb.lo);
            out_w[g] = cnt;
        }
    }
}

static int launch_abx_count(const aew_abx_count_t& p, hipStream_t st) {
    const int rc = abx_check(p, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_abx_count, dim3((unsigned)p.N), dim3(ABX_WAVES * 64), (size_t)p.N * sizeof(float), st, p);
    return (int)hipGetLastError();
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------
extern "C" int aew_abx_host(const aew_abx_count_t* pp) {
    if (!pp) return AEW_E_ARG;
    const aew_abx_count_t& p = *pp;
    const int rc = abx_check(p, true);
    if (rc) return rc;
    const int N = p.N, G = p.G;
    std::vector<float> row((size_t)N);
    std::vector<int> group_of((size_t)N);
    for (int g = 0; g < G; ++g)
        for (int x = p.groups_host[g].lo; x < p.groups_host[g].hi; ++x) group_of[x] = g;
    for (int x = 0; x < N; ++x) {                                                 // what one workgroup does
        const float* drow = p.dist + (int64_t)p.perm_host[x] * p.ld;
        for (int j = 0; j < N; ++j) row[j] = drow[p.perm_host[j]];
        const int gx = group_of[x];
        for (int g = 0; g < G; ++g) {
            const aew_abx_group_t gb = p.groups_host[g];
            int alo = 0, ahi = 0, self = 0;
            uint32_t n = 0, cnt = 0;
            if (abx_cell(p.groups_host, p.partner_host, N, G, p.C, p.S, p.mode, gx, gb, &alo, &ahi, &self)) {
                for (int b = gb.lo; b < gb.hi; ++b) {
                    for (int a = alo; a < ahi; ++a) cnt += abx_w(row[a], row[b]);
                    if (self) cnt -= abx_w(row[x], row[b]);
                }
                n = (uint32_t)(ahi - alo - self) * (uint32_t)(gb.hi - gb.lo);
            }
            p.n[(int64_t)x * G + g] = n;
            p.wrong2[(int64_t)x * G + g] = cnt;
        }
    }
    return 0;
}
