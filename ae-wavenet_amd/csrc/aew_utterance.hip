// aew_utterance.hip — whole utterances through the fixed-geometry encoder: AEW_OP_MEL_TILE fills the engine's mel input
// with windows cut out of a ragged buffer of whole-utterance mels (zeros behind the frames that exist), AEW_OP_CODE_STITCH
// moves the codes of a batch to their place in the ragged outputs.  Both read one device-resident table of aew_utt_row_t
// (aewavenet.h states the contract).  Byte movers: plain loads and stores, no atomics, every loop bounded by the record.
// Part of the library's one translation unit (aewavenet.hip includes it).
#pragma once
#include "aew_common.h"

// ---- what the whole-utterance files share (this one is included first; aew_cond_utterance.hip and aew_score.hip follow)
// the table of a tile or stitch record: a device copy the kernel reads and a host copy the launcher checks, aligned to 8
// bytes for aew_utt_row_t and to 16 for aew_cond_row_t / aew_score_row_t
template <typename Row>
static int tile_table_check(const Row* table, const Row* host, int first_row, int B) {
    if (!table || !host || B < 1 || B > 65535 || first_row < 0) return AEW_E_ARG;
    if (((uintptr_t)table | (uintptr_t)host) & (std::is_same<Row, aew_utt_row_t>::value ? 7 : 15)) return AEW_E_ALIGN;
    return 0;
}
// the launchers' walk over the host copy of the batch's rows: n_of is the record's check, negative for a row it refuses
template <typename P, typename F>
static bool tile_rows_ok(const P& p, F n_of) {
    for (int b = 0; b < p.B; ++b)
        if (n_of(p.table_host[(int64_t)p.first_row + b]) < 0) return false;
    return true;
}
// the code window aew_cond_row_t and aew_score_row_t share: the codes that are read - hi - lo - or -1 for a window
// AEW_OP_CODE_TILE and AEW_OP_WAV_TILE refuse: the reads of a good one stay inside [0, n_codes)
template <typename Row>
__host__ __device__ __forceinline__ int32_t code_window_n(const Row& r, int E, int64_t n_codes, int n_voice) {
    if (r.lo < 0 || r.hi < r.lo || r.hi > E || r.voice < 0 || r.voice >= n_voice) return -1;
    if (r.hi > r.lo) {
        if (r.code0 < -(int64_t)E || r.code0 > n_codes) return -1;              // (keeps the sums below far from overflow)
        if (r.code0 + r.lo < 0 || r.code0 + r.hi > n_codes) return -1;
    }
    return r.hi - r.lo;
}
// the cut of batch row b's code window by the STRIDE threads of a block, for a record p with codes / ind / E / K
// (aew_code_tile_t, aew_wav_tile_t): ind[b][j] = codes[code0 + j] for j in [lo, hi) of a live row, code 0 elsewhere and
// where the code lies outside [0, K).  -> this thread's count of such codes; the caller adds it to its own counter and
// stores the row's voice behind that
template <int STRIDE, typename P, typename Row>
__device__ __forceinline__ unsigned int code_window_cut(const P& p, const Row& r, bool live, int b) {
    int64_t* ind = p.ind + (int64_t)b * p.E;
    unsigned int bad = 0;
    for (int j = threadIdx.x; j < p.E; j += STRIDE) {
        int64_t c = 0;
        if (live && j >= r.lo && j < r.hi) {
            c = p.codes[r.code0 + j];
            if (c < 0 || c >= (int64_t)p.K) { c = 0; ++bad; }
        }
        ind[j] = c;
    }
    return bad;
}

// ---- the index arithmetic, ONE definition for the kernels, the launchers' checks and aew_utterance_locate (the CPU tests
// run this very code)
// frames of the row's window that exist, or -1 for a record AEW_OP_MEL_TILE refuses: the reads of a good record stay
// inside [0, n_src), element (n_mel - 1) * pitch + avail - 1 behind src being the last one
__host__ __device__ __forceinline__ int32_t utt_tile_avail(const aew_utt_row_t& r, int n_mel, int mel_len, int64_t n_src) {
    if (r.avail < 0 || r.avail > mel_len) return -1;
    if (r.avail == 0) return 0;
    if (r.src < 0 || r.pitch < r.avail) return -1;
    const int64_t span = (int64_t)(n_mel - 1) * r.pitch + r.avail;
    return (span <= n_src && r.src <= n_src - span) ? r.avail : -1;
}
// codes of the row that are stored, or -1 for a record AEW_OP_CODE_STITCH refuses: the writes of a good record stay
// inside [0, n_dst)
__host__ __device__ __forceinline__ int32_t utt_stitch_n(const aew_utt_row_t& r, int E, int64_t n_dst) {
    if (r.n_valid < 0 || r.n_valid > E) return -1;
    if (r.n_valid == 0) return 0;
    return (r.dst >= 0 && r.n_valid <= n_dst && r.dst <= n_dst - r.n_valid) ? r.n_valid : -1;
}
// element i of in_mel[b] (row-major (n_mel, mel_len)): its source element in the ragged buffer, or -1 for a zero
__host__ __device__ __forceinline__ int64_t utt_src(const aew_utt_row_t& r, int32_t avail, int mel_len, int64_t i) {
    const int64_t c = i / mel_len;
    const int32_t t = (int32_t)(i - c * mel_len);
    return t < avail ? r.src + c * r.pitch + t : -1;
}

extern "C" int aew_utterance_locate(const aew_utt_row_t* row, int n_mel, int mel_len, int E, int64_t n_src, int64_t n_dst,
                                    int64_t i, int64_t* src, int32_t* avail, int32_t* n_valid) {
    if (!row || !src || !avail || !n_valid || n_mel < 1 || mel_len < 1 || E < 1 || n_src < 0 || n_dst < 0 || i < 0 ||
        i >= (int64_t)n_mel * mel_len)
        return AEW_E_ARG;
    const int32_t a = utt_tile_avail(*row, n_mel, mel_len, n_src), n = utt_stitch_n(*row, E, n_dst);
    if (a < 0 || n < 0) return AEW_E_ARG;
    *avail = a; *n_valid = n; *src = utt_src(*row, a, mel_len, i);
    return 0;
}

// ---- AEW_OP_MEL_TILE
#define AEW_UTT_THREADS 256

// One destination quad (VEC: 16 bytes of the 16-byte aligned, multiple-of-4 long in_mel[b]) or one element per thread.
// A window's first frame is only 4-byte aligned in the ragged buffer, so the source side takes the widest load its
// address allows - 16, 8 or 4 bytes - when the quad lies in one channel and all four frames exist; a quad that straddles
// a channel seam or the end of the frames goes element by element.  A record that fails the launcher's check (the table
// changed under a captured graph) is treated as idle: the row becomes zeros, nothing outside [0, n_src) is read.
template <bool VEC>
__global__ __launch_bounds__(AEW_UTT_THREADS) void k_mel_tile(const aew_mel_tile_t p) {
    const int b = blockIdx.y;
    const aew_utt_row_t r = p.table[(int64_t)p.first_row + b];
    int32_t avail = utt_tile_avail(r, p.n_mel, p.mel_len, p.n_src);
    if (avail < 0) avail = 0;
    const int64_t row_n = (int64_t)p.n_mel * p.mel_len;
    float* dst = p.in_mel + (int64_t)b * row_n;
    const int64_t q = (int64_t)blockIdx.x * AEW_UTT_THREADS + threadIdx.x;
    if constexpr (VEC) {
        const int64_t i0 = 4 * q;
        if (i0 >= row_n) return;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int32_t t0 = (int32_t)(i0 % p.mel_len);
        if (t0 + 3 < p.mel_len && t0 + 3 < avail) {          // one channel, four frames that exist
            const float* s = p.mel + utt_src(r, avail, p.mel_len, i0);
            const uintptr_t a = (uintptr_t)s;
            if ((a & 15) == 0) v = *reinterpret_cast<const float4*>(s);
            else if ((a & 7) == 0) {
                const float2 lo = *reinterpret_cast<const float2*>(s), hi = *reinterpret_cast<const float2*>(s + 2);
                v = make_float4(lo.x, lo.y, hi.x, hi.y);
            } else v = make_float4(s[0], s[1], s[2], s[3]);
        } else {
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t so = utt_src(r, avail, p.mel_len, i0 + k);
                e[k] = so >= 0 ? p.mel[so] : 0.f;
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        }
        *reinterpret_cast<float4*>(dst + i0) = v;
    } else {
        if (q >= row_n) return;
        const int64_t so = utt_src(r, avail, p.mel_len, q);
        dst[q] = so >= 0 ? p.mel[so] : 0.f;
    }
}

static int launch_mel_tile(const aew_mel_tile_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.mel || !p.in_mel || p.n_mel < 1 || p.mel_len < 1 || p.n_src < 0) return AEW_E_ARG;
    if (((uintptr_t)p.mel | (uintptr_t)p.in_mel) & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return utt_tile_avail(r, p.n_mel, p.mel_len, p.n_src); })) return AEW_E_ARG;
    const int64_t row_n = (int64_t)p.n_mel * p.mel_len;
    const bool vec = !(row_n & 3) && !((uintptr_t)p.in_mel & 15);
    const int64_t per_row = vec ? row_n / 4 : row_n;
    const dim3 grid((unsigned)((per_row + AEW_UTT_THREADS - 1) / AEW_UTT_THREADS), (unsigned)p.B);
    hipLaunchKernelGGL(vec ? k_mel_tile<true> : k_mel_tile<false>, grid, dim3(AEW_UTT_THREADS), 0, st, p);
    return (int)hipGetLastError();
}

// ---- AEW_OP_CODE_STITCH
// One wave per row: the first n_valid of the row's E codes (and distances) go to dst, element by element - the destination
// offset is any multiple of the element size, so 8 bytes (int64) and 4 bytes (fp32) are the widest accesses both sides
// allow.  A record that fails the launcher's check stores nothing.
__global__ __launch_bounds__(AEW_WAVE) void k_code_stitch(const aew_code_stitch_t p) {
    const int b = blockIdx.x;
    const aew_utt_row_t r = p.table[(int64_t)p.first_row + b];
    const int32_t n = utt_stitch_n(r, p.E, p.n_dst);
    const int64_t* ind = p.ind + (int64_t)b * p.E;
    for (int j = threadIdx.x; j < n; j += AEW_WAVE) p.codes[r.dst + j] = ind[j];
    if (p.dist) {
        const float* md = p.min_dist + (int64_t)b * p.E;
        for (int j = threadIdx.x; j < n; j += AEW_WAVE) p.dist[r.dst + j] = md[j];
    }
}

static int launch_code_stitch(const aew_code_stitch_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.ind || !p.codes || p.E < 1 || p.n_dst < 0 || (p.dist && !p.min_dist)) return AEW_E_ARG;
    if (((uintptr_t)p.ind | (uintptr_t)p.codes) & 7) return AEW_E_ALIGN;
    if (((uintptr_t)p.min_dist | (uintptr_t)p.dist) & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return utt_stitch_n(r, p.E, p.n_dst); })) return AEW_E_ARG;
    hipLaunchKernelGGL(k_code_stitch, dim3((unsigned)p.B), dim3(AEW_WAVE), 0, st, p);
    return (int)hipGetLastError();
}

// ---- AEW_OP_FRAME_STITCH
// The encoder outputs of a batch to their place in the ragged frame buffer: the first n_valid rows (d_pitch floats each)
// of batch row b go to the rows dst .. of `frames` - one contiguous run of n_valid * d_pitch elements on both sides.
// VEC: 16-byte moves (d_pitch and lin_bs multiples of 4, both buffers 16-byte aligned, so every run starts on 16 bytes).
// The same record check as AEW_OP_CODE_STITCH; a record that fails it stores nothing.
template <bool VEC>
__global__ __launch_bounds__(AEW_UTT_THREADS) void k_frame_stitch(const aew_frame_stitch_t p) {
    const int b = blockIdx.y;
    const aew_utt_row_t r = p.table[(int64_t)p.first_row + b];
    const int32_t n = utt_stitch_n(r, p.E, p.n_dst);
    if (n <= 0) return;
    const int64_t total = (int64_t)n * p.d_pitch;
    const float* src = p.lin + (int64_t)b * p.lin_bs;
    float* dst = p.frames + r.dst * p.d_pitch;
    const int64_t q = (int64_t)blockIdx.x * AEW_UTT_THREADS + threadIdx.x;
    if constexpr (VEC) {
        if (4 * q < total) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(src)[q];
    } else {
        if (q < total) dst[q] = src[q];
    }
}

static int launch_frame_stitch(const aew_frame_stitch_t& p, hipStream_t st) {
    int rc = tile_table_check(p.table, p.table_host, p.first_row, p.B);
    if (rc) return rc;
    if (!p.lin || !p.frames || p.E < 1 || p.d_pitch < 1 || p.n_dst < 0 || p.lin_bs < (int64_t)p.E * p.d_pitch) return AEW_E_ARG;
    if (((uintptr_t)p.lin | (uintptr_t)p.frames) & 3) return AEW_E_ALIGN;
    if (!tile_rows_ok(p, [&](auto& r) { return utt_stitch_n(r, p.E, p.n_dst); })) return AEW_E_ARG;
    const bool vec = !(p.d_pitch & 3) && !(p.lin_bs & 3) && !(((uintptr_t)p.lin | (uintptr_t)p.frames) & 15);
    const int64_t per_row = (int64_t)p.E * p.d_pitch / (vec ? 4 : 1);
    const dim3 grid((unsigned)((per_row + AEW_UTT_THREADS - 1) / AEW_UTT_THREADS), (unsigned)p.B);
    hipLaunchKernelGGL(vec ? k_frame_stitch<true> : k_frame_stitch<false>, grid, dim3(AEW_UTT_THREADS), 0, st, p);
    return (int)hipGetLastError();
}
