// aew_evalgroups.hip — evaluation by group (aew_eval_groups_t): the per-window sums of the evaluation accumulator
// folded into a record indexed by a per-window group id, the (group, code) contingency table, and the finalize that
// reads the per-group means and the mutual information I(code; group) off them.  Every floating sum follows the order
// written in the header (eval_tree of aew_ops.hip is THE tree); plain loads, double additions and integer atomics only;
// no workgroup waits on another - the steps of a launch are separate kernels on one stream.
#include "aew_common.h"

// =============================================================================================
// accumulate, per window: workgroup b owns window b.  Thread t adds the window's positions u = t, t + 1024, ... ascending
// (four per pass, loads first) and its queries j = t, t + 1024, ...; the window's queries are counted in row group[b] of
// the table unless the window is dropped.  win[b] = S(nll), S(ptgt), hits, S(dist).
// =============================================================================================
__global__ __launch_bounds__(1024) void k_evg_window(const aew_eval_groups_t p) {
    __shared__ double sh[1024];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t g = p.group[b];
    const bool live = g >= 0 && g < (int64_t)p.G;
    double s_nll = 0.0, s_pt = 0.0, s_hit = 0.0, s_d = 0.0;
    if (p.nll) {
        const int wl = p.w - 1;
        const float* nll = p.nll + b * p.w;
        const float* ptgt = p.ptgt + b * p.w;
        const float* wav = p.wav + b * p.wav_pitch + p.tgt_off + 1;
        for (int u0 = t; u0 < wl; u0 += 4096) {
            float vn[4], vp[4], hit[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int u = u0 + 1024 * r;
                vn[r] = vp[r] = hit[r] = 0.f;
                if (u >= wl) continue;
                vn[r] = nll[u];
                vp[r] = ptgt[u];
                const int tgt = (int)wav[u];
                int am = 0;
                if (p.amax) am = p.amax[b * p.w + u];
                else {
                    const float* lg = p.logits + b * p.bs + (int64_t)u * p.pitch;
                    float best = lg[0];
                    for (int c = 1; c < p.n_quant; ++c) {
                        const float v = lg[c];
                        if (v > best) { best = v; am = c; }    // strictly greater: the lowest class keeps a tie
                    }
                }
                hit[r] = am == tgt ? 1.f : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (u0 + 1024 * r < wl) { s_nll += (double)vn[r]; s_pt += (double)vp[r]; s_hit += (double)hit[r]; }
        }
    }
    if (p.ind) {
        const int64_t q0 = b * p.Qw;
        uint32_t* row = live ? p.ghist + g * (int64_t)p.K : nullptr;      // (64-bit: G * K reaches 10^6 and more)
        for (int j = t; j < p.Qw; j += 1024) {
            if (p.dist) s_d += (double)p.dist[q0 + j];
            const int64_t k = p.ind[q0 + j];
            if (live && k >= 0 && k < (int64_t)p.K) atomicAdd(row + k, 1u);   // integer: exact whatever the order
        }
    }
    const double w_nll = eval_tree(sh, s_nll), w_pt = eval_tree(sh, s_pt), w_hit = eval_tree(sh, s_hit);
    const double w_d = eval_tree(sh, s_d);
    if (t == 0) {
        double* o = p.win + 4 * b;
        o[0] = w_nll; o[1] = w_pt; o[2] = w_hit; o[3] = w_d;
    }
}

// =============================================================================================
// accumulate, per group: thread g walks the windows ascending and adds those of its group to gacc[g], one double
// addition per entry; the thread of group 0 also counts the dropped windows and the batch.
// =============================================================================================
__global__ __launch_bounds__(256) void k_evg_fold(const aew_eval_groups_t p) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.G) return;
    double* a = p.gacc + AEW_EVAL_GACC_N * g;
    double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6];
    const double n_pos = p.nll ? (double)(p.w - 1) : 0.0;
    double dropped = 0.0;
    for (int b = 0; b < p.B; ++b) {
        const int64_t gb = p.group[b];
        if (gb < 0 || gb >= (int64_t)p.G) dropped += 1.0;
        if (gb != g) continue;
        const double* s = p.win + 4 * (int64_t)b;
        a0 += 1.0;
        a1 += n_pos;
        if (p.nll) { a2 += s[0]; a3 += s[1]; a4 += s[2]; }
        if (p.ind) {
            a5 += (double)p.Qw;
            if (p.dist) a6 += s[3];
        }
    }
    a[0] = a0; a[1] = a1; a[2] = a2; a[3] = a3; a[4] = a4; a[5] = a5; a[6] = a6;
    if (g == 0) { p.gtot[0] += dropped; p.gtot[1] += 1.0; }
}

// =============================================================================================
// finalize.  Scratch: cols uint64 [K] (the column sums n_k), then rows double [G][4] (n_g, E_g, J_g, cells_g).
//   k_evg_cols   the integer column sums: a wave reads 64 consecutive words of a row, four waves split the rows
//   k_evg_rows   workgroup g: n_g, N, then E_g and J_g in THE order over k; writes gout[g] and rows[g]
//   k_evg_total  one workgroup: H(C) in THE order over k; the rows' terms in parallel, added ascending g by thread 0; writes tout
// =============================================================================================
#define AEW_EVG_COLS 64                                        // codes per workgroup of k_evg_cols (one wave wide)
__global__ __launch_bounds__(256) void k_evg_cols(const aew_eval_groups_t p) {
    // four waves share 64 columns: wave s takes the rows s, s + 4, ... (eight loads in flight, each a 256-byte row
    // segment per wave), the four partial counts meet in LDS.  Integer sums: exact in any order.
    __shared__ unsigned long long part[4][AEW_EVG_COLS];
    const int lane = threadIdx.x & (AEW_EVG_COLS - 1), slice = threadIdx.x / AEW_EVG_COLS;
    const int64_t k = (int64_t)blockIdx.x * AEW_EVG_COLS + lane;
    unsigned long long c = 0;
    if (k < p.K) {
        const uint32_t* col = p.ghist + k;
        int g = slice;
        for (; g + 28 < p.G; g += 32) {
            uint32_t h[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) h[r] = col[(int64_t)(g + 4 * r) * p.K];
#pragma unroll
            for (int r = 0; r < 8; ++r) c += h[r];
        }
        for (; g < p.G; g += 4) c += col[(int64_t)g * p.K];
    }
    part[slice][lane] = c;
    __syncthreads();
    if (slice == 0 && k < p.K)
        static_cast<unsigned long long*>(p.scratch)[k] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

__device__ __forceinline__ double evg_div(double x, double y) { return y > 0.0 ? x / y : 0.0; }

__global__ __launch_bounds__(1024) void k_evg_rows(const aew_eval_groups_t p) {
    __shared__ double shd[1024];
    __shared__ unsigned long long shn[1024];
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;
    unsigned long long n_g = 0, cells = 0, N = 0;
    double ent = 0.0, J = 0.0;
    if (p.ghist) {
        const uint32_t* row = p.ghist + g * (int64_t)p.K;
        const unsigned long long* cols = static_cast<const unsigned long long*>(p.scratch);
        unsigned long long n = 0, used = 0, tot = 0;
        for (int k = t; k < p.K; k += 1024) { const uint32_t h = row[k]; n += h; used += h > 0u ? 1u : 0u; tot += cols[k]; }
        n_g = eval_tree(shn, n); cells = eval_tree(shn, used); N = eval_tree(shn, tot);
        double e = 0.0, j = 0.0;
        if (n_g > 0)
            for (int k = t; k < p.K; k += 1024) {
                const uint32_t h = row[k];
                if (h == 0u) continue;
                const double pr = (double)h / (double)n_g;
                e -= pr * log2(pr);
                j += (double)h * log2(((double)h * (double)N) / ((double)n_g * (double)cols[k]));
            }
        ent = eval_tree(shd, e);
        J = eval_tree(shd, j);
    }
    if (t != 0) return;
    const double* a = p.gacc + AEW_EVAL_GACC_N * g;
    float* o = p.gout + AEW_EVAL_GOUT_N * g;
    const double nll = evg_div(a[2], a[1]);
    o[0] = (float)a[0];
    o[1] = (float)a[1];
    o[2] = (float)nll;
    o[3] = (float)(nll / 0.693147180559945309417232121458);
    o[4] = (float)evg_div(a[4], a[1]);
    o[5] = (float)evg_div(a[3], a[1]);
    o[6] = (float)evg_div(a[6], a[5]);
    o[7] = (float)a[5];
    o[8] = (float)ent;
    o[9] = n_g > 0 ? (float)exp2(ent) : 0.f;
    o[10] = (float)cells;
    o[11] = 0.f;
    if (p.ghist) {
        double* r = static_cast<double*>(p.scratch) + p.K + 4 * g;
        r[0] = (double)n_g; r[1] = ent; r[2] = J; r[3] = (double)cells;
    }
}

__global__ __launch_bounds__(1024) void k_evg_total(const aew_eval_groups_t p) {
    __shared__ double st[5][1024];                            // the trees' scratch, then the staged row terms
    double* shd = st[0];
    unsigned long long* shn = reinterpret_cast<unsigned long long*>(st[1]);
    const int t = threadIdx.x;
    unsigned long long N = 0, n_cols = 0;
    double hc = 0.0;
    if (p.ghist) {
        const unsigned long long* cols = static_cast<const unsigned long long*>(p.scratch);
        unsigned long long n = 0, used = 0;
        for (int k = t; k < p.K; k += 1024) { const unsigned long long c = cols[k]; n += c; used += c > 0 ? 1u : 0u; }
        N = eval_tree(shn, n); n_cols = eval_tree(shn, used);
        double e = 0.0;
        if (N > 0)
            for (int k = t; k < p.K; k += 1024) {
                const unsigned long long c = cols[k];
                if (c > 0) { const double pr = (double)c / (double)N; e -= pr * log2(pr); }
            }
        hc = eval_tree(shd, e);
    }
    float* o = p.tout;
    if (!p.ghist) {
        if (t == 0) {
            for (int i = 0; i < AEW_EVAL_TOUT_N; ++i) o[i] = 0.f;
            o[11] = (float)p.gtot[0];
            o[12] = (float)p.gtot[1];
        }
        return;
    }
    // the sums over g: every thread computes the terms of one row (the log2 is the expensive part), thread 0 adds them
    // ascending g - one adder, one order - 1024 rows at a time
    const double* rows = static_cast<const double*>(p.scratch) + p.K;
    const double dN = (double)N;
    double hg = 0.0, hcg = 0.0, jsum = 0.0, cells = 0.0, n_rows = 0.0;
    for (int base = 0; base < p.G; base += 1024) {
        const int g = base + t;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};              // p_g log2 p_g, p_g E_g, J_g, cells_g, row used
        if (g < p.G) {
            const double* r = rows + 4 * (int64_t)g;
            if (r[0] > 0.0) {
                const double pg = r[0] / dN;
                v[0] = pg * log2(pg); v[1] = pg * r[1]; v[2] = r[2]; v[3] = r[3]; v[4] = 1.0;
            }
        }
        __syncthreads();                                      // (the trees' readers, the fold of the rows before)
#pragma unroll
        for (int i = 0; i < 5; ++i) st[i][t] = v[i];
        __syncthreads();
        if (t == 0) {
            const int n = p.G - base < 1024 ? p.G - base : 1024;
            for (int i = 0; i < n; ++i) {
                if (st[4][i] == 0.0) continue;                // rows with n_g == 0 are skipped
                hg -= st[0][i];
                hcg += st[1][i];
                jsum += st[2][i];
                cells += st[3][i];
                n_rows += 1.0;
            }
        }
    }
    if (t != 0) return;
    const double mi = evg_div(jsum, dN);
    const double mm = N > 0 ? mi - (cells - n_rows - (double)n_cols + 1.0) / (2.0 * dN * 0.693147180559945309417232121458) : 0.0;
    o[0] = (float)dN;
    o[1] = (float)hc;
    o[2] = (float)hg;
    o[3] = (float)hcg;
    o[4] = (float)mi;
    o[5] = (float)mm;
    o[6] = (float)evg_div(mi, hg);
    o[7] = (float)evg_div(mi, hc);
    o[8] = (float)cells;
    o[9] = (float)n_rows;
    o[10] = (float)n_cols;
    o[11] = (float)p.gtot[0];
    o[12] = (float)p.gtot[1];
    o[13] = o[14] = o[15] = 0.f;
}

static int launch_eval_groups(const aew_eval_groups_t& p, hipStream_t st) {
    if (p.G < 1 || !p.gacc || !p.gtot) return AEW_E_ARG;
    if (p.finalize) {
        if (!p.gout || !p.tout || (p.ghist && (p.K < 1 || !p.scratch))) return AEW_E_ARG;
    } else {
        if (p.B < 1 || !p.group || !p.win) return AEW_E_ARG;
        if (p.ind && (p.K < 1 || p.Qw < 1 || !p.ghist)) return AEW_E_ARG;
        if (!p.nll) {
            if (!p.ind) return AEW_E_ARG;                     // codes-only counts queries: there must be some
        } else {
            if (p.w < 2 || !p.ptgt || !p.wav) return AEW_E_ARG;
            if (!p.amax && (!p.logits || p.n_quant < 1)) return AEW_E_ARG;
        }
    }
    if (((uintptr_t)p.gacc | (uintptr_t)p.gtot | (uintptr_t)p.win | (uintptr_t)p.ind | (uintptr_t)p.group | (uintptr_t)p.scratch) & 7)
        return AEW_E_ALIGN;
    if (((uintptr_t)p.nll | (uintptr_t)p.ptgt | (uintptr_t)p.wav | (uintptr_t)p.amax | (uintptr_t)p.logits | (uintptr_t)p.dist |
         (uintptr_t)p.ghist | (uintptr_t)p.gout | (uintptr_t)p.tout) & 3) return AEW_E_ALIGN;
    if (p.finalize) {
        if (p.ghist) hipLaunchKernelGGL(k_evg_cols, dim3((unsigned)((p.K + AEW_EVG_COLS - 1) / AEW_EVG_COLS)), dim3(256), 0, st, p);
        hipLaunchKernelGGL(k_evg_rows, dim3((unsigned)p.G), dim3(1024), 0, st, p);
        hipLaunchKernelGGL(k_evg_total, dim3(1), dim3(1024), 0, st, p);
    } else {
        hipLaunchKernelGGL(k_evg_window, dim3((unsigned)p.B), dim3(1024), 0, st, p);
        hipLaunchKernelGGL(k_evg_fold, dim3((unsigned)((p.G + 255) / 256)), dim3(256), 0, st, p);
    }
    return (int)hipGetLastError();
}
