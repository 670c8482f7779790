// zsw_score.hip — score / score+ends kernels for gfx950 (MI355X).
//
// What is computed: for every read (the profile sequence, "query") the Smith-Waterman affine-gap
// local score against the context's reference, i.e. the value sw_simd_score returns
// (reference: src/alignment/sw/striped.rs:65-142) and, in ENDS mode, the (ref_end, query_end) of
// sw_simd_score_ends (striped.rs:213-336: first row holding the maximum, then first column).
// Both are invariant to Zoe's SIMD lane count N (they equal the Gotoh recurrence that
// src/alignment/sw/scalar.rs:55-122 states), so this kernel is free to parallelise differently:
//
//   * inter-read: each 32-bit lane carries TWO reads as packed i16 (v_pk_add_i16/v_pk_sub_i16 with
//     clamp = Zoe's saturating_add/sub, v_pk_max_i16); scores live at offset i16::MIN exactly as in
//     Zoe's signed profiles, so saturation at MIN is the zero floor of local alignment;
//   * a group of G adjacent lanes owns one read pair; lane g keeps columns [g*C, (g+1)*C) of H and E
//     in VGPRs and walks down the reference one row per step, skewed by g steps (anti-diagonal
//     wavefront at strip granularity); the only cross-lane traffic is the strip's last H and F, one
//     wave shuffle each per step;
//   * the reference row's four substitution scores (8 bytes) come from an LDS table built once per
//     block; the per-column score is ONE v_perm_b32 of that row by a per-column selector register
//     that encodes the two reads' residues — no per-cell memory access at all.
//
// 10 VALU instructions per packed cell pair; no MFMA (this is not a contraction); HBM traffic is the
// read bytes in and 4-5 bytes out per read. The binding roof is integer VALU issue.
#include <stdlib.h>

#include <algorithm>

#include "zsw_internal.hpp"
#include "zsw_score_v1.hpp"
#include "zsw_score_prune.hpp"
#include "zsw_score_seed.hpp"
#include "zsw_score_v2.hpp"
#include "zsw_handback.hpp"
#include "zsw_timer.hpp"

namespace zsw {

// Exact 32-bit kernel: any alphabet size, any read length, no saturation below 2^31. One thread per
// read, H/E rows in global scratch ([column][slot], coalesced over threads). Used for reads whose
// packed-i16 score saturated, for alphabets the table kernels do not cover (S > 7) and for reads
// longer than the largest strip configuration. Follows scalar.rs:55-122 (same recurrence, same
// strict-greater scan order = first row, then first column).
__global__ __launch_bounds__(64) void exact32_kernel(BatchDev b, const uint32_t* list, const uint32_t* list_count,
                                                     const uint8_t* ref, uint32_t ref_len, const ScoringDev* sc,
                                                     ResultRule rule, ScoreOut out, int32_t* scratch, uint32_t slots,
                                                     uint32_t scratch_len, const uint32_t* rev_ref_end,
                                                     const uint32_t* rev_query_end) {
    __shared__ uint8_t lut[256];
    __shared__ int32_t w[MAX_S * MAX_S];
    for (int i = threadIdx.x; i < 256; i += 64) lut[i] = sc->index_map[i];
    for (int i = threadIdx.x; i < MAX_S * MAX_S; i += 64) w[i] = sc->w[i];
    __syncthreads();
    const int S = sc->S;
    const int go = sc->gap_open, ge = sc->gap_extend;
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    const uint32_t n = list ? *list_count : b.n_items;
    int32_t* Hrow = scratch + slot;
    int32_t* Erow = scratch + (size_t)slots * scratch_len + slot;
    for (uint32_t item = slot; item < n; item += slots) {
        const uint32_t id = list ? list[item] : (b.items ? b.items[item] : item);
        uint64_t off;
        uint32_t len;
        if (b.offsets) {
            off = b.offsets[id];
            len = (uint32_t)(b.offsets[id + 1] - off);
        } else {
            off = (uint64_t)id * b.fixed_len;
            len = b.fixed_len;
        }
        uint32_t rows = ref_len;
        if (rev_ref_end) {  // reverse pass of sw_simd_score_ranges: reversed prefixes of both sequences
            len = rev_query_end[id] <= len ? rev_query_end[id] : len;
            rows = len ? rev_ref_end[id] : 0;
        }
        if (len == 0 || len > scratch_len) {
            out.score[id] = 0;
            out.status[id] = len == 0 ? ZSW_STATUS_EMPTY : ZSW_STATUS_OVERFLOWED;
            if (out.tier) out.tier[id] = 0;
            if (out.ref_end) out.ref_end[id] = 0;
            if (out.query_end) out.query_end[id] = 0;
            continue;
        }
        for (uint32_t c = 0; c < len; ++c) {
            Hrow[(size_t)c * slots] = 0;
            Erow[(size_t)c * slots] = 0;
        }
        int64_t best = 0;
        uint32_t r_end = 0, c_end = 0;
        for (uint32_t r = 0; r < rows; ++r) {
            const int32_t* wr = &w[lut[ref[rev_ref_end ? rows - 1 - r : r]] * S];
            int32_t f = 0, diag = 0;
            for (uint32_t c = 0; c < len; ++c) {
                const int32_t up = Hrow[(size_t)c * slots];
                int32_t e = Erow[(size_t)c * slots];
                int32_t h = diag + wr[lut[b.bases[rev_ref_end ? off + (len - 1 - c) : off + c]]];
                h = max(max(h, e), max(f, 0));
                if (h > best) {
                    best = h;
                    r_end = r;
                    c_end = c;
                }
                Hrow[(size_t)c * slots] = h;
                e = max(max(e - ge, h - go), 0);
                f = max(max(f - ge, h - go), 0);
                Erow[(size_t)c * slots] = e;
                diag = up;
            }
        }
        uint32_t score;
        uint8_t status, tier;
        apply_rule(rule, (uint64_t)best, &score, &status, &tier);
        out.score[id] = score;
        out.status[id] = status;
        if (out.tier) out.tier[id] = tier;
        const bool some = status == ZSW_STATUS_SOME;
        if (rev_ref_end) {  // inclusive starts
            out.ref_end[id] = some ? rows - (r_end + 1) : 0;
            out.query_end[id] = some ? len - (c_end + 1) : 0;
        } else {
            if (out.ref_end) out.ref_end[id] = some ? r_end + 1 : 0;
            if (out.query_end) out.query_end[id] = some ? c_end + 1 : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
using Cfg = StripCfg;
// strip configurations, ascending capacity G*C
#define ZSW_CFG_ENTRY(GV, CV) {GV, CV},
static const Cfg kCfgs[] = {ZSW_FOR_EACH_STRIP_CONFIG(ZSW_CFG_ENTRY)};
#undef ZSW_CFG_ENTRY

constexpr int N_ASCENDING_CFGS = 20;  // the rest of kCfgs is for small batches only (score_config_for_batch)
constexpr int N_CFGS = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));

bool score_config_for(uint32_t max_len, int* G, int* C) { return strip_config_first_fit(kCfgs, N_ASCENDING_CFGS, max_len, G, C); }

// Same, for a batch of n_items reads (zsw_handback.hpp: strip_config_for_batch).
static bool score_config_for_batch(uint32_t max_len, uint32_t n_items, int* G, int* C) {
    return strip_config_for_batch(kCfgs, N_CFGS, max_len, n_items, G, C);
}

template <int G, int C>
static hipError_t launch_cfg(const ScoreArgs& a, bool fast, int mode, hipStream_t stream) {
    const uint32_t reads_per_block = 2 * (BLOCK / G);
    const uint32_t grid = (a.b.n_items + reads_per_block - 1) / reads_per_block;
    if (grid == 0) return hipSuccess;
#define ZSW_LAUNCH(FASTV, MODEV) hipLaunchKernelGGL((score_kernel<G, C, FASTV, MODEV>), dim3(grid), dim3(BLOCK), 0, stream, a)
    if (fast) {
        if (mode == 0) ZSW_LAUNCH(true, 0);
        else if (mode == 1) ZSW_LAUNCH(true, 1);
        else ZSW_LAUNCH(true, 2);
    } else {
        if (mode == 0) ZSW_LAUNCH(false, 0);
        else if (mode == 1) ZSW_LAUNCH(false, 1);
        else ZSW_LAUNCH(false, 2);
    }
#undef ZSW_LAUNCH
    return hipGetLastError();
}

// Chooses the table form. FAST needs every query residue code >= 4 to score 0 against every
// reference residue (true for S <= 4, and for DNA matrices built with `ignoring = Some(b'N')`).
static bool fast_ok(const ScoringDev& s) {
    if (s.S > 8) return false;
    for (int r = 0; r < s.S; ++r)
        for (int q = 4; q < s.S; ++q)
            if (s.w[r * s.S + q] != 0) return false;
    return true;
}

// the largest weight of the matrix (0 if none is positive)
static int max_weight(const ScoringDev& s) {
    int maxw = 0;
    for (int i = 0; i < s.S * s.S; ++i) maxw = std::max(maxw, (int)s.w[i]);
    return maxw;
}

static void build_tables(const ScoringDev& s, bool fast, ScoreArgs* a) {
    int bias = 0;
    for (int i = 0; i < s.S * s.S; ++i) bias = s.w[i] < -bias ? -s.w[i] : bias;
    auto pk = [](uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | (hi << 16); };
    for (int r = 0; r < 9; ++r) {
        uint32_t lo = 0, hi = 0;
        if (fast) {
            int v[4] = {0, 0, 0, 0};
            if (r < s.S)
                for (int q = 0; q < 4 && q < s.S; ++q) v[q] = s.w[r * s.S + q];
            lo = pk((uint32_t)v[0], (uint32_t)v[1]);
            hi = pk((uint32_t)v[2], (uint32_t)v[3]);
        } else {
            uint8_t by[8];
            for (int q = 0; q < 8; ++q) by[q] = (uint8_t)bias;
            if (r < s.S)
                for (int q = 0; q < s.S && q < 7; ++q) by[q] = (uint8_t)(s.w[r * s.S + q] + bias);
            lo = by[0] | (by[1] << 8) | (by[2] << 16) | ((uint32_t)by[3] << 24);
            hi = by[4] | (by[5] << 8) | (by[6] << 16) | ((uint32_t)by[7] << 24);
        }
        a->wtab[r][0] = lo;
        a->wtab[r][1] = hi;
    }
    a->go2 = pk((uint32_t)s.gap_open, (uint32_t)s.gap_open);
    a->ge2 = pk((uint32_t)s.gap_extend, (uint32_t)s.gap_extend);
    a->bias2 = pk((uint32_t)bias, (uint32_t)bias);
}

template <int G, int C>
static hipError_t launch_cfg_v2(const ScoreArgsV2& a, int mode, hipStream_t stream) {
    const uint32_t reads_per_block = 2 * (BLOCK / G);
    const uint32_t grid = (a.b.n_items + reads_per_block - 1) / reads_per_block;
    if (grid == 0) return hipSuccess;
    const dim3 g(grid, a.chunk_rows ? (a.ref_len + a.chunk_rows - 1) / a.chunk_rows : 1u);  // row-chunked launches: one grid row per chunk
    if (mode == 0) hipLaunchKernelGGL((score_kernel_v2<G, C, 0>), g, dim3(BLOCK), 0, stream, a);
    else if (mode == 1) hipLaunchKernelGGL((score_kernel_v2<G, C, 1>), g, dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((score_kernel_v2<G, C, 2>), g, dim3(BLOCK), 0, stream, a);
    return hipGetLastError();
}

// Row-chunked launches (ScoreArgsV2::chunk_rows): the keys of the listed reads before, their results after.
__global__ void chunk_zero_kernel(const uint32_t* items, const uint32_t* n_dev, uint32_t n_max, unsigned long long* keys) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < min(*n_dev, n_max)) keys[items[i]] = 0ull;
}
__global__ void chunk_finalize_kernel(BatchDev b, const uint32_t* n_dev, const unsigned long long* keys, uint32_t limit, ResultRule rule, ScoreOut out, int mode) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(*n_dev, b.n_items)) return;
    const uint32_t id = b.items[i];
    const uint32_t len = b.offsets ? (uint32_t)(b.offsets[id + 1] - b.offsets[id]) : b.fixed_len;
    const unsigned long long key = keys[id];
    const uint32_t s = (uint32_t)(key >> (CHUNK_ROW_BITS + CHUNK_COL_BITS));
    const uint32_t row1 = ((1u << CHUNK_ROW_BITS) - 1u) - (uint32_t)((key >> CHUNK_COL_BITS) & ((1u << CHUNK_ROW_BITS) - 1u));
    const uint32_t col1 = ((1u << CHUNK_COL_BITS) - 1u) - (uint32_t)(key & ((1u << CHUNK_COL_BITS) - 1u));
    if (len == 0) {
        out.score[id] = 0;
        out.status[id] = ZSW_STATUS_EMPTY;
        if (out.tier) out.tier[id] = 0;
        if (mode != 0 && out.ref_end) out.ref_end[id] = 0;
        if (mode == 2 && out.query_end) out.query_end[id] = 0;
    } else if (s >= limit) {  // near the representable limit: recompute exactly in 32 bits (not reached behind seed_applicable, which
                              // requires maxw * max_len + 8 < limit: no read of a seeded class can score that much; kept as the rule of
                              // score_kernel_v2's own epilogue, and there is no test for it)
        out.fb_list[atomicAdd(out.fb_count, 1u)] = id;
    } else {
        uint32_t score;
        uint8_t status, tier;
        apply_rule(rule, (uint64_t)s, &score, &status, &tier);
        out.score[id] = score;
        out.status[id] = status;
        if (out.tier) out.tier[id] = tier;
        const bool some = status == ZSW_STATUS_SOME;
        if (mode != 0 && out.ref_end) out.ref_end[id] = some ? row1 : 0;
        if (mode == 2 && out.query_end) out.query_end[id] = some ? col1 : 0;
    }
}

static hipError_t launch_table_cfg_v2(const ScoreArgsV2& a, int G, int C, int mode, hipStream_t stream) {
    switch (G * 100 + C) {
#define ZSW_CASE(GV, CV) \
    case GV * 100 + CV: return launch_cfg_v2<GV, CV>(a, mode, stream);
        ZSW_FOR_EACH_STRIP_CONFIG(ZSW_CASE)
#undef ZSW_CASE
    }
    return hipErrorInvalidValue;
}

// (zsw_score_seed.hpp: the slices of the hand-back list are launched from zsw_score_seed.hip)
hipError_t launch_score_v2_cfg(const ScoreArgsV2& a, int G, int C, int mode, hipStream_t stream) { return launch_table_cfg_v2(a, G, C, mode, stream); }

// v2 needs: S <= 7; for query residues 0..3: s + ge in [-128, 127]; for residues >= 4: s + ge in [0, 255].
static bool v2_ok(const ScoringDev& s, uint32_t debug) {
    if (debug & ZSW_DEBUG_SCORE_V1) return false;
    if (s.S > 7) return false;
    for (int r = 0; r < s.S; ++r)
        for (int q = 0; q < s.S; ++q) {
            const int t = s.w[r * s.S + q] + s.gap_extend;
            if (q < 4 ? (t < -128 || t > 127) : (t < 0 || t > 255)) return false;
        }
    return true;
}

// Drift-domain constants for strip width G; returns false if the drifted range does not leave room for scores.
static bool v2_range_setup(const ScoringDev& s, int G, ScoreArgsV2* a) {
    const int ge = s.gap_extend, go = s.gap_open;
    a->ge2 = (uint32_t)ge * 0x00010001u;
    a->gd2 = (uint32_t)(go - ge) * 0x00010001u;
    uint32_t K = 2048;
    while (K > 16 && K * (uint32_t)ge > 8192) K /= 2;
    a->K = K;
    a->floor0 = 1152u + (uint32_t)G * (uint32_t)ge + 128u;
    const uint32_t dmax = a->floor0 + (K + 2) * (uint32_t)ge;
    if (dmax + 1024 > 0x7C00u - 512u) return false;
    a->limit = 0x7C00u - 512u - dmax;
    return true;
}

// Fills the v2 tables for strip width G (alphabets of up to 7 letters).
static bool build_tables_v2(const ScoringDev& s, int G, ScoreArgsV2* a) {
    const int ge = s.gap_extend;
    for (int r = 0; r < 9; ++r) {
        uint8_t by[8];
        for (int q = 0; q < 8; ++q) by[q] = (uint8_t)ge;  // true 0 (+ge): padding, unused slots and the neutral row
        if (r < s.S)
            for (int q = 0; q < s.S; ++q) {
                const int t = s.w[r * s.S + q] + ge;
                if (q < 4) by[2 * q + 1] = (uint8_t)(int8_t)t;
                else by[2 * (q - 3)] = (uint8_t)t;
            }
        a->wtab[r][0] = by[0] | (by[1] << 8) | (by[2] << 16) | ((uint32_t)by[3] << 24);
        a->wtab[r][1] = by[4] | (by[5] << 8) | (by[6] << 16) | ((uint32_t)by[7] << 24);
    }
    return v2_range_setup(s, G, a);
}

// The banded seeded kernel's tables: every weight and gap penalty doubled (strip width 1: a lane owns whole strips). false when the
// doubled weights do not fit the table bytes.
static bool doubled_tables(const ScoringDev& s, ScoreArgsV2* a) {
    ScoringDev d = s;
    for (int i = 0; i < s.S * s.S; ++i) d.w[i] = 2 * s.w[i];
    d.gap_open = 2 * s.gap_open;
    d.gap_extend = 2 * s.gap_extend;
    return v2_ok(d, 0) && build_tables_v2(d, 1, a);
}

// WIDE kernels: 8..32 letters, every score + ge must fit a signed byte.
static bool wide_ok(const ScoringDev& s, uint32_t debug) {
    if (debug & ZSW_DEBUG_NO_WIDE) return false;
    if (s.S <= 7 || s.S > 32) return false;
    for (int i = 0; i < s.S * s.S; ++i) {
        const int t = s.w[i] + s.gap_extend;
        if (t < -128 || t > 127) return false;
    }
    return true;
}

static void fill_wide_table(const ScoringDev& s, ScoreArgsV2* a) {
    const int ge = s.gap_extend;
    for (int r = 0; r < 33; ++r)
        for (int q = 0; q < WIDE_STRIDE; ++q)
            a->wide[r * WIDE_STRIDE + q] = (int8_t)((r < s.S && q < s.S) ? s.w[r * s.S + q] + ge : ge);
}

static bool build_tables_wide(const ScoringDev& s, int G, ScoreArgsV2* a) {
    fill_wide_table(s, a);
    return v2_range_setup(s, G, a);
}

// The 32-bit tile kernel takes any alphabet of up to 32 letters whose weights + gap_extend fit a signed byte, as long as the
// drifted values stay inside an i32 for this reference and read length.
static bool w32_ok(const ScoringDev& s, uint32_t ref_len, uint32_t max_len, uint32_t debug) {
    if ((debug & ZSW_DEBUG_NO_W32) || s.S > 32) return false;
    for (int i = 0; i < s.S * s.S; ++i) {
        const int t = s.w[i] + s.gap_extend;
        if (t < -128 || t > 127) return false;
    }
    const uint64_t top = ((uint64_t)ref_len + TILE_G + 4) * (uint64_t)s.gap_extend + (uint64_t)max_len * (uint64_t)max_weight(s);
    return top < 0x7f000000ull;
}

static hipError_t launch_table_cfg(const ScoreArgs& a, int G, int C, bool fast, int mode, hipStream_t stream) {
    switch (G * 100 + C) {
#define ZSW_CASE(GV, CV) \
    case GV * 100 + CV: return launch_cfg<GV, CV>(a, fast, mode, stream);
        ZSW_FOR_EACH_STRIP_CONFIG(ZSW_CASE)
#undef ZSW_CASE
    }
    return hipErrorInvalidValue;
}

// ---- ragged batches: group the reads by the smallest strip configuration that holds them -------------------
// class k < NCLS: kCfgs[kBucketCfg[k]]; class NCLS: longer than every table configuration (exact 32-bit kernel)
static const int kBucketCfg[] = {0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19};  // (8,19) duplicates the capacity of (4,38)
constexpr int NCLS = 19;

struct BucketCaps {
    uint32_t cap[NCLS];
};

__device__ __forceinline__ int bucket_of(const BucketCaps& caps, uint32_t len) {
    int k = 0;
    while (k < NCLS && len > caps.cap[k]) ++k;
    return k;
}

__global__ void reverse_bytes_kernel(const uint8_t* in, uint32_t n, uint8_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[n - 1 - i];
}

__global__ void iota_kernel(uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

__global__ void bucket_count_kernel(const uint64_t* offsets, uint32_t n, BucketCaps caps, uint32_t* counts) {
    __shared__ uint32_t sh[NCLS + 1];
    if (threadIdx.x <= NCLS) sh[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        atomicAdd(&sh[bucket_of(caps, (uint32_t)(offsets[i + 1] - offsets[i]))], 1u);
    __syncthreads();
    if (threadIdx.x <= NCLS && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

__global__ void bucket_scatter_kernel(const uint64_t* offsets, uint32_t n, BucketCaps caps, uint32_t* cursors, uint32_t* items) {
    // one atomic per wavefront and class (a million single atomics on twenty cursors took 3.2 ms)
    const int lane = threadIdx.x & 63;
    const uint32_t per_sweep = gridDim.x * blockDim.x;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += per_sweep) {
        const uint32_t i = base + threadIdx.x;
        const bool valid = i < n;
        const int k = valid ? bucket_of(caps, (uint32_t)(offsets[i + 1] - offsets[i])) : -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int kl = __shfl(k, leader, 64);
            const unsigned long long same = __ballot(valid && k == kl);
            if (k == kl) {
                uint32_t start = 0;
                if (lane == leader) start = atomicAdd(&cursors[kl], (uint32_t)__popcll(same));
                start = (uint32_t)__shfl((int)start, leader, 64);
                items[start + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = i;
            }
            todo &= ~same;
        }
    }
}

__global__ void add_count_kernel(const uint32_t* count, uint32_t* total) { atomicAdd(total, *count); }

// ZSW_OPTION_MIN_SCORE, the exact-score route: behind every kernel of launch_score, whichever scored a read. A read that is
// UNMAPPED, or SOME with a score below min_thr (= min(T, the last tier's overflow threshold): an OVERFLOWED read never is), becomes
// BELOW_MIN_SCORE with every other field 0 — what the seed kernel and the band tiers wrote for the reads their bounds settled.
// Grid-stride, one atomic per wavefront at the end.
__global__ void min_filter_kernel(BatchDev b, uint32_t min_thr, ScoreOut out, uint32_t* count) {
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n_items; i += gridDim.x * blockDim.x) {
        const uint32_t id = b.items ? b.items[i] : i;
        const uint8_t st = out.status[id];
        if (st == ZSW_STATUS_UNMAPPED || (st == ZSW_STATUS_SOME && out.score[id] < min_thr)) {
            out.score[id] = 0;
            out.status[id] = ZSW_STATUS_BELOW_MIN_SCORE;
            if (out.tier) out.tier[id] = 0;
            if (out.ref_end) out.ref_end[id] = 0;
            if (out.query_end) out.query_end[id] = 0;
            ++mine;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}

// ---- the score dispatcher ------------------------------------------------------------------------------------------------------
// What one call of launch_score / launch_score_rev is about: filled once, const from then on. Every step below builds the ScoreArgs
// or ScoreArgsV2 it launches as a copy of v1 / v2 — no table set is shared scratch — and takes the stream it launches on as a
// parameter: no step decides a stream for another.
struct ScoreCall {
    const ScoringDev* d_sc;
    const ScoringDev& h_sc;
    const BatchDev& b;
    uint32_t max_len;
    const uint8_t* d_ref;
    uint32_t ref_len;
    const ResultRule& rule;
    const ScoreOut& out;
    const ScoreWorkspace& ws;
    int mode, maxw;
    bool wide, fast, table_ok, use_v2;
    uint32_t exact_grid;
    // (value-initialised: the reverse pass's pointers, the tile fields and whatever else a step does not set are null)
    ScoreArgs v1;    // the fields every launch shares, and score_kernel's tables where it can serve the call
    ScoreArgsV2 v2;  // the fields every launch shares; each step adds the tables of its strip width

    ScoreCall(const ScoringDev* d_sc, const ScoringDev& h_sc, const BatchDev& b, uint32_t max_len, const uint8_t* d_ref, uint32_t ref_len,
              const ResultRule& rule, const ScoreOut& out, const ScoreWorkspace& ws, int mode)
        : d_sc(d_sc), h_sc(h_sc), b(b), max_len(max_len), d_ref(d_ref), ref_len(ref_len), rule(rule), out(out), ws(ws), mode(mode), v1{}, v2{} {
        wide = wide_ok(h_sc, ws.debug);
        fast = fast_ok(h_sc);
        table_ok = h_sc.S <= 7 || fast || wide;
        use_v2 = table_ok && !wide && v2_ok(h_sc, ws.debug);
        exact_grid = (uint32_t)(ws.slots / 64);
        maxw = max_weight(h_sc);
        common(&v1);
        if (table_ok && !wide) build_tables(h_sc, fast, &v1);
        common(&v2);
    }

  private:
    template <class Args>
    void common(Args* a) const {
        a->b = b;
        a->ref = d_ref;
        a->ref_len = ref_len;
        a->sc = d_sc;
        a->rule = rule;
        a->out = out;
    }
};

// What a call leaves behind from one step to the next.
struct ScoreDispatch {
    const ScoreCall call;
    bool seed_gtabs_built = false;  // ws.seed_gtab holds the call's per-row tables (build_seed_gtabs)
};

// The exact 32-bit kernel over the items of `bb`, or over those of them that `list` names (the worklist); rev_*: the reverse pass.
static hipError_t launch_exact32(const ScoreCall& c, const BatchDev& bb, const uint32_t* list, const uint32_t* list_count, const uint32_t* rev_ref_end,
                                 const uint32_t* rev_query_end, hipStream_t stream) {
    note_launch(c.ws.launch_log, list ? ZSW_LAUNCH_EXACT32_WORKLIST : ZSW_LAUNCH_EXACT32, 0, 0, std::min(c.mode, 2));
    hipLaunchKernelGGL(exact32_kernel, dim3(c.exact_grid), dim3(64), 0, stream, bb, list, list_count, c.d_ref, c.ref_len, c.d_sc, c.rule, c.out,
                       c.ws.scratch, (uint32_t)c.ws.slots, c.ws.scratch_len, rev_ref_end, rev_query_end);
    return hipGetLastError();
}

static hipError_t launch_one(const ScoreCall& c, const BatchDev& bb, int g, int cc, hipStream_t stream) {
    std::vector<uint32_t>* const launches = c.ws.launch_log;  // zsw_debug_score_launches
    if (c.wide || c.use_v2) {
        ScoreArgsV2 a2 = c.v2;
        a2.b = bb;
        if (c.wide) {
            if (!build_tables_wide(c.h_sc, g, &a2)) return launch_exact32(c, bb, nullptr, nullptr, nullptr, nullptr, stream);
            if (bb.n_items) note_launch(launches, ZSW_LAUNCH_WIDE, g, cc, c.mode == 0 ? 0 : 2);
            return launch_table_cfg_v2_wide(a2, g, cc, c.mode, stream);
        }
        if (build_tables_v2(c.h_sc, g, &a2)) {
            if (bb.n_items) note_launch(launches, ZSW_LAUNCH_V2, g, cc, std::min(c.mode, 2));
            return launch_table_cfg_v2(a2, g, cc, c.mode, stream);
        }
    }
    ScoreArgs a = c.v1;
    a.b = bb;
    if (bb.n_items) note_launch(launches, c.fast ? ZSW_LAUNCH_V1_FAST : ZSW_LAUNCH_V1_BIASED, g, cc, std::min(c.mode, 2));
    return launch_table_cfg(a, g, cc, c.fast, c.mode, stream);
}

// The tile kernels hand the strip boundary of every reference row from tile to tile through the two halves of ws.tile_buf: the
// items a round can take, with one boundary per pair (the packed tiles: per_entry 2) or per read (the 32-bit ones: 1). 0: none fits.
static uint32_t tile_round_items(const ScoreCall& c, uint32_t per_entry, uint32_t n_items) {
    const size_t per = (size_t)c.ref_len * sizeof(uint2);
    const size_t fit = per ? c.ws.tile_bytes / 2 / per : (size_t)n_items;
    return (uint32_t)std::min<size_t>(per_entry * fit, per_entry == 2 ? 0x7ffffffeu : 0x7fffffffu);
}

// n_items items in rounds of per_round, each round tile by tile over `longest` columns, ping-pong between the halves of tile_buf.
// launch_tile(a, first) launches one tile of the round that begins at item `first`: `a` holds the round's item count and the tile's
// columns and buffers; where the items come from is the caller's (a.b.items, or the list it passes to launch_tile_w32).
template <class LaunchTile>
static hipError_t tile_rounds(const ScoreCall& c, ScoreArgsV2 a, uint32_t n_items, uint32_t per_round, uint32_t longest, uint32_t kind, LaunchTile launch_tile) {
    uint2* buf[2] = {c.ws.tile_buf, reinterpret_cast<uint2*>(reinterpret_cast<uint8_t*>(c.ws.tile_buf) + c.ws.tile_bytes / 2)};
    const uint32_t n_tiles = (longest + TILE_COLS - 1) / TILE_COLS;
    a.tile_state = c.ws.tile_state;
    for (uint32_t first = 0; first < n_items; first += per_round) {
        a.b.n_items = std::min<uint32_t>(per_round, n_items - first);
        for (uint32_t t = 0; t < n_tiles; ++t) {
            a.tile_q0 = t * (uint32_t)TILE_COLS;
            a.tile_in = t ? buf[(t - 1) & 1] : nullptr;
            a.tile_out = t + 1 < n_tiles ? buf[t & 1] : nullptr;
            note_launch(c.ws.launch_log, kind, TILE_G, TILE_C, c.mode == 0 ? 0 : 2);
            hipError_t e = launch_tile(a, first);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// Reads longer than the widest strip configuration: TILE_COLS query columns per launch, the strip boundary of every
// reference row handed from tile to tile through HBM, as many reads per round as the boundary buffers hold.
// Returns hipErrorNotSupported when the packed kernels cannot take the batch (the caller then uses the exact kernel).
static hipError_t launch_tiled(const ScoreCall& c, const BatchDev& bb, uint32_t longest, hipStream_t stream) {
    const ScoreWorkspace& ws = c.ws;
    if (!ws.tile_buf || !ws.tile_state || !bb.items || (ws.debug & ZSW_DEBUG_NO_TILES)) return hipErrorNotSupported;
    if (!(c.wide || c.use_v2)) return hipErrorNotSupported;
    ScoreArgsV2 a2 = c.v2;
    if (!(c.wide ? build_tables_wide(c.h_sc, TILE_G, &a2) : build_tables_v2(c.h_sc, TILE_G, &a2))) return hipErrorNotSupported;
    const uint32_t per_round = tile_round_items(c, 2, bb.n_items);
    if (per_round == 0) return hipErrorNotSupported;
    a2.b = bb;
    return tile_rounds(c, a2, bb.n_items, per_round, longest, c.wide ? ZSW_LAUNCH_TILE_WIDE : ZSW_LAUNCH_TILE_V2, [&](ScoreArgsV2& a, uint32_t first) {
        a.b.items = bb.items + first;
        return launch_tile_v2(a, c.wide, c.mode, stream);
    });
}

// The arguments of the 32-bit tile kernel (before the tile fields): any alphabet w32_ok admits, in the WIDE table
static ScoreArgsV2 w32_args(const ScoreCall& c) {
    ScoreArgsV2 a2 = c.v2;
    fill_wide_table(c.h_sc, &a2);
    a2.ge2 = (uint32_t)c.h_sc.gap_extend * 0x00010001u;
    a2.gd2 = (uint32_t)(c.h_sc.gap_open - c.h_sc.gap_extend) * 0x00010001u;
    return a2;
}

// Reads whose score is beyond the packed range sit in the device-side worklist (usually empty). Batches that can hold such
// scores at all (long reads) read the count back and run the 32-bit tile kernel over the list; everything else launches the
// exact kernel on the worklist unconditionally, which keeps short-read calls asynchronous.
static hipError_t finish_worklist(const ScoreCall& c, hipStream_t stream) {
    const ScoreWorkspace& ws = c.ws;
    if ((uint64_t)c.max_len * (uint64_t)std::max(c.maxw, 1) >= 16384 && ws.tile_buf && ws.tile_state && w32_ok(c.h_sc, c.ref_len, c.max_len, ws.debug)) {
        uint32_t cnt = 0;
        hipError_t we = hipMemcpyAsync(&cnt, c.out.fb_count, sizeof(cnt), hipMemcpyDeviceToHost, stream);
        if (we == hipSuccess) we = hipStreamSynchronize(stream);
        if (we != hipSuccess) return we;
        if (cnt == 0) return hipSuccess;
        const uint32_t per_round = tile_round_items(c, 1, cnt);
        if (per_round)
            return tile_rounds(c, w32_args(c), cnt, per_round, c.max_len, ZSW_LAUNCH_TILE_W32,
                               [&](const ScoreArgsV2& a, uint32_t first) { return launch_tile_w32(a, c.out.fb_list + first, c.mode, stream); });
    }
    return launch_exact32(c, c.b, c.out.fb_list, c.out.fb_count, nullptr, nullptr, stream);
}

// The seeded pass's per-row score tables, for blocks whose windows do not fit one LDS table (same bytes for every strip width),
// once per call: `plain` from the call's tables, `band` (null: no banded kernel) from the doubled ones.
static hipError_t build_seed_gtabs(ScoreDispatch& d, const ScoreArgsV2& plain, const ScoreArgsV2* band, hipStream_t stream) {
    if (d.seed_gtabs_built) return hipSuccess;
    hipError_t e = seed_build_gtab(plain, d.call.ws.seed_gtab, stream);
    if (e == hipSuccess && band) e = seed_build_gtab(*band, seed_gtab_band(d.call.ws, d.call.ref_len), stream);
    d.seed_gtabs_built = e == hipSuccess;
    return e;
}

// Against a long reference the few reads handed back are cut into chunks of rows, each an item of its own (a class of
// 2,000 reads walking 30,000 rows each is a dozen blocks on 256 CUs): chunks of at least four times the rows a
// positive path can span, so that the overlap costs a quarter more cells at most. (tests/chunk_edge_reads.py restates the rule.)
struct RowChunks {
    uint64_t rows, overlap;
    bool enabled;
};
static RowChunks row_chunks_for(const ScoreCall& c, uint32_t longest) {
    const ScoringDev& s = c.h_sc;
    RowChunks r;
    r.overlap = s.gap_extend > 0 ? (uint64_t)longest + (uint64_t)longest * (uint64_t)c.maxw / (uint64_t)s.gap_extend + 2 : ~0ull;
    r.rows = std::max<uint64_t>(4 * r.overlap, 2048);
    r.enabled = c.ws.chunk_keys && !(c.ws.debug & ZSW_DEBUG_NO_ROW_CHUNKS) && s.gap_extend > 0 && r.rows * 2 <= c.ref_len && longest < (1u << CHUNK_COL_BITS) &&
                c.ref_len < (1u << CHUNK_ROW_BITS) - 2;
    return r;
}

// The full pass over the hand-back list of a seeded range (ap: the range's tables, its list and count), in chunks of rows.
// (never co-scheduled: chunk_finalize_kernel writes the result of every read of the list)
static hipError_t score_handed_back_chunked(const ScoreCall& c, ScoreArgsV2 ap, const RowChunks& rc, int g, int cc, uint32_t n_items, hipStream_t stream) {
    ap.chunk_rows = (uint32_t)rc.rows;
    ap.chunk_overlap = (uint32_t)rc.overlap;
    ap.chunk_keys = c.ws.chunk_keys;
    const uint32_t zgrid = (n_items + 255) / 256;
    hipLaunchKernelGGL(chunk_zero_kernel, dim3(zgrid), dim3(256), 0, stream, ap.b.items, ap.n_items_dev, n_items, c.ws.chunk_keys);
    note_launch(c.ws.launch_log, ZSW_LAUNCH_ROW_CHUNKS, (int)ap.chunk_rows, (int)ap.chunk_overlap, (int)((c.ref_len + ap.chunk_rows - 1) / ap.chunk_rows));
    note_launch(c.ws.launch_log, ZSW_LAUNCH_V2, g, cc, std::min(c.mode, 2));
    hipError_t pe = launch_table_cfg_v2(ap, g, cc, c.mode, stream);
    if (pe != hipSuccess) return pe;
    hipLaunchKernelGGL(chunk_finalize_kernel, dim3(zgrid), dim3(256), 0, stream, ap.b, ap.n_items_dev, c.ws.chunk_keys, ap.limit, c.rule, c.out, std::min(c.mode, 2));
    return hipGetLastError();
}

// ... or over whole rows. A short list is latency-bound in the class's configuration (10,000 reads hand back a few hundred: one
// wavefront per 32 reads walking all R rows is 1.3 ms whatever the count), a long one throughput-bound in any other. The count
// stays on the device, so the list is launched in up to three configurations — the ones the cost model picks for
// 16 k, 128 k and many reads — and each launch returns at once unless the count lies in its range (measured, 1 M
// reads: 21 k handed back 1.27 ms at 8 lanes per pair, 1.1 ms at 16; 110 k: 4.3 ms at 4 lanes, 4.0 ms at 8).
// (zsw_handback.hpp: the plan, and the invariant tests/models/handback_plan.cpp holds it to.)
static hipError_t score_handed_back_gated(const ScoreCall& c, const ScoreArgsV2& ap, int g, int cc, uint32_t longest, uint32_t n_items, hipStream_t stream) {
    HandbackLaunch plan[HANDBACK_MAX_LAUNCHES];
    ScoreArgsV2 tabs[HANDBACK_MAX_LAUNCHES];
    int n_tabs = 0;
    const int n_plan = handback_plan(kCfgs, N_CFGS, longest, g, cc, n_items, [&](int g2) {
        tabs[n_tabs] = c.v2;
        if (!build_tables_v2(c.h_sc, g2, &tabs[n_tabs])) return false;
        ++n_tabs;
        return true;
    }, plan);
    hipError_t pe = hipSuccess;
    for (int k = 0, t = 0; k < n_plan && pe == hipSuccess; ++k) {
        ScoreArgsV2 ah = ap;
        if (plan[k].own_tables) {  // (tables_ok succeeded once per such launch, in the plan's order)
            ah = tabs[t++];
            ah.b = ap.b;
            ah.n_items_dev = ap.n_items_dev;
            ah.first_item_dev = ap.first_item_dev;  // (the gates choose by the remainder)
        }
        ah.b.n_items = plan[k].grid_items;
        ah.gate_lo = plan[k].lo;
        ah.gate_hi = plan[k].hi;
        note_launch(c.ws.launch_log, ZSW_LAUNCH_V2, plan[k].G, plan[k].C, std::min(c.mode, 2));
        pe = launch_table_cfg_v2(ah, plan[k].G, plan[k].C, c.mode, stream);
    }
    return pe;
}

// Seeded exact pass (zsw_score_seed.hip) over the items of `bb` in strip configuration (g, cc): seed + sort + band or window kernel,
// then score_kernel_v2 over the reads it hands back (device-side list; `counter` = its count, zeroed here). The workspace region
// [work_off, work_off + seed_workspace_bytes(n_items)) and fail_list + list_off belong to this call alone.
// slice_streams: non-null = `stream` is the caller's own (the one-length route) and slices of the co-scheduled hand-back list may
// run on slice_streams->s[0] (head) and s[1] (tail), forked from and joined to `stream` here (zsw_handback.hpp: handback_slices).
// hipErrorNotSupported: not switched on, or the batch does not qualify.
static hipError_t seed_items(ScoreDispatch& d, const BatchDev& bb, int g, int cc, uint32_t longest, size_t work_off, uint32_t list_off, uint32_t* counter,
                             uint32_t band_grid_cap, const SideStreams* slice_streams, hipStream_t stream) {
    const ScoreCall& c = d.call;
    const ScoreWorkspace& ws = c.ws;
    if (!c.use_v2 || !ws.seed || !ws.seed_work || !ws.prune_fail_list || !(ws.debug & ZSW_DEBUG_SCORE_PRUNE) || (ws.debug & ZSW_DEBUG_PRUNE_STRIP))
        return hipErrorNotSupported;
    if (bb.n_items < SEED_MIN_READS && !(ws.debug & ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE)) return hipErrorNotSupported;
    const size_t work_bytes = seed_workspace_bytes(bb.n_items, longest, band_grid_cap);
    if (g == 32 || work_off + work_bytes > ws.seed_bytes) return hipErrorNotSupported;
    ScoreArgsV2 ap = c.v2;
    if (!build_tables_v2(c.h_sc, g, &ap) || !seed_applicable(*ws.seed, longest, c.ref_len, ap.limit)) return hipErrorNotSupported;
    if (!ws.seed_gtab) return hipErrorNotSupported;
    // the banded kernel works on doubled scores (zsw_seed.hpp: an odd value marks a path through a cell outside the band): its own
    // drift constants and per-row table, if the doubled weights fit the table bytes
    ScoreArgsV2 ab = c.v2;
    const ScoreArgsV2* const band = !(ws.debug & ZSW_DEBUG_SEED_NO_BAND) && doubled_tables(c.h_sc, &ab) ? &ab : nullptr;
    hipError_t pe = build_seed_gtabs(d, ap, band, stream);
    if (pe != hipSuccess) return pe;
    pe = hipMemsetAsync(counter, 0, 4, stream);
    if (pe != hipSuccess) return pe;
    ap.b = bb;
    const RowChunks rc = row_chunks_for(c, longest);
    static_assert(2 + NCLS <= 32, "the n0 words sit 32 behind their counters");
    static_assert(2 + NCLS <= 32 - HANDBACK_BOUND_WORDS, "the slice bounds take the last words behind the n0 words");
    // (ws.prune_fail_count: 64 words, the counters in the first 2 + NCLS, the n0 word of each 32 behind it, the slice bounds of the
    // one-length route — whose counter is word 0 — in the last HANDBACK_BOUND_WORDS)
    const SeedRegion region = {ws.seed_work + work_off, work_bytes, ws.prune_fail_list + list_off, counter, counter + 32};
    // Slices of the co-scheduled list: the rule as if the decision held (launch_score_seeded applies it only then). The tail runs in
    // the class's own configuration with its tables (zsw_handback.hpp: the register budget).
    HandbackSliceLaunch sl{};
    sl.rule = handback_slice_rule(true, slice_streams != nullptr && counter == ws.prune_fail_count, bb.n_items, (ws.debug & ZSW_DEBUG_SEED_NO_SLICES) != 0,
                                  (ws.debug & ZSW_DEBUG_SEED_TINY_SLICES) != 0);
    const bool slices = sl.rule.head() || sl.rule.tail();
    ScoreArgsV2 tail_tabs = c.v2;
    if (slices) {
        sl.bounds = ws.prune_fail_count + 64 - HANDBACK_BOUND_WORDS;
        sl.head = slice_streams->s[0];
        sl.tail = slice_streams->s[1];
        sl.seeded = slice_streams->seeded;
        sl.shared = slice_streams->shared;
        sl.tail_tabs = &ap;
        sl.tail_G = g;
        sl.tail_C = cc;
        // HANDBACK_TAIL_G lanes per pair, if that is not the class's own: the narrowest such row that holds the reads, with its
        // tables (as score_handed_back_gated builds them); none, or no tables: the class's configuration
        for (int k = 0; k < N_ASCENDING_CFGS && HANDBACK_TAIL_G != g && sl.tail_G == g; ++k) {
            if (kCfgs[k].G != HANDBACK_TAIL_G || (uint32_t)(kCfgs[k].G * kCfgs[k].C) < longest || !build_tables_v2(c.h_sc, kCfgs[k].G, &tail_tabs)) continue;
            tail_tabs.b = bb;
            sl.tail_tabs = &tail_tabs;
            sl.tail_G = kCfgs[k].G;
            sl.tail_C = kCfgs[k].C;
        }
    }
    bool coscheduled = false;
    pe = launch_score_seeded(ap, g, cc, longest, ws, region, c.mode, band, band_grid_cap, rc.enabled, &coscheduled, slices ? &sl : nullptr, stream);
    if (pe != hipSuccess) return pe;
    // out.skip_handed_back (the shared-profile role's passes, the seeded reverse pass of the ranges): the caller recomputes every
    // read without the `unique` flag by other means, the handed-back reads among them — scoring them here would be thrown away
    if (c.out.skip_handed_back) return hipSuccess;
    ap.b.items = region.fail_list;
    ap.n_items_dev = counter;
    ap.first_item_dev = coscheduled ? region.n0 : nullptr;  // (not co-scheduled: n0 is not written, and nothing changes)
    pe = rc.enabled ? score_handed_back_chunked(c, ap, rc, g, cc, bb.n_items, stream) : score_handed_back_gated(c, ap, g, cc, longest, bb.n_items, stream);
    if (pe != hipSuccess) return pe;
    // the slices join here, behind the caller's own launches (which they ran beside) and in front of everything that reads what a
    // slice wrote: its results, and the saturation worklist it may have appended to (finish_worklist)
    if (coscheduled && slices) {
        for (int i = 0; i < 2; ++i) {
            if (!(i == 0 ? sl.rule.head() : sl.rule.tail())) continue;
            pe = hipEventRecord(slice_streams->join[i], slice_streams->s[i]);
            if (pe == hipSuccess) pe = hipStreamWaitEvent(stream, slice_streams->join[i], 0);
            if (pe != hipSuccess) return pe;
        }
    }
    // zsw_prune_rescored counts the reads scored over all their cells HERE: a pass whose handed-back reads the caller settles by
    // other means (the reversed pass of the ranges, the shared role's ends) adds nothing
    hipLaunchKernelGGL(add_count_kernel, dim3(1), dim3(1), 0, stream, counter, ws.prune_fail_count + 1);
    return hipGetLastError();
}

// Column-pruned pass over the items of `bb` (reads of at most kPruneClasses[cls].max_len bases), then score_kernel_v2 over the
// reads it hands back (device-side list and count). hipErrorNotSupported: not switched on, or the batch does not qualify.
static hipError_t prune_items(const ScoreCall& c, const BatchDev& bb, int cls, uint32_t n_cls, hipStream_t stream) {
    const ScoreWorkspace& ws = c.ws;
    const bool wide = c.wide;
    // 5-letter tables: behind ZSW_DEBUG_PRUNE_STRIP (the seeded pass is their default); 8..32 letter alphabets (WIDE tables): the
    // default first pass — the seeded pass's k-mer argument does not hold for matrices whose substitutions score close to identities
    if (!(c.use_v2 || wide) || !ws.prune_work || !(ws.debug & ZSW_DEBUG_SCORE_PRUNE)) return hipErrorNotSupported;
    if (!wide && !(ws.debug & ZSW_DEBUG_PRUNE_STRIP)) return hipErrorNotSupported;
    if (bb.n_items < PR_MIN_READS && !(ws.debug & ZSW_DEBUG_SCORE_PRUNE_ANY_SIZE)) return hipErrorNotSupported;
    const int last = n_cls < bb.n_items ? cls + 1 : cls;  // the range may hold the next class too (same strip width)
    ScoreArgsV2 ap = c.v2;
    auto tables = [&](int g, ScoreArgsV2* t) { return wide ? build_tables_wide(c.h_sc, g, t) : build_tables_v2(c.h_sc, g, t); };
    if (!tables(1, &ap)) return hipErrorNotSupported;
    const uint32_t floor_strip = ap.floor0;
    uint32_t limit = ap.limit, floor_window[2] = {0, 0};
    for (int k = cls; k <= last; ++k) {
        if (!tables(kPruneClasses[k].g, &ap)) return hipErrorNotSupported;
        floor_window[k - cls] = ap.floor0;
        limit = std::min(limit, ap.limit);
    }
    if (!prune_applicable(c.h_sc, kPruneClasses[last].max_len, c.ref_len, limit)) return hipErrorNotSupported;
    int Gr = 0, Cr = 0;
    if (!score_config_for(kPruneClasses[last].max_len, &Gr, &Cr)) return hipErrorNotSupported;
    hipError_t pe = hipMemsetAsync(ws.prune_fail_count, 0, 4, stream);
    if (pe != hipSuccess) return pe;
    ap.b = bb;
    uint32_t est_failed = 0xffffffffu;
    pe = launch_score_pruned(ap, cls, n_cls, floor_strip, floor_window, c.h_sc, ws.prune_work, ws.prune_bytes, ws.prune_chunk,
                             ws.prune_fail_list, ws.prune_fail_count, c.mode, wide, stream, &est_failed);
    if (pe != hipSuccess) return pe;
    note_launch(ws.launch_log, ZSW_LAUNCH_PRUNED, kPruneClasses[cls].g, kPruneClasses[cls].cp, std::min(c.mode, 2));
    // a short list of handed-back reads is latency-bound in the narrowest configuration (20,000 reads of 150 residues: 3.4 ms
    // at four lanes per pair, every block walking all R rows): with the probe's estimate it takes the small-batch configuration
    if (est_failed != 0xffffffffu) (void)score_config_for_batch(kPruneClasses[last].max_len, est_failed + est_failed / 4 + 1024, &Gr, &Cr);
    if (!tables(Gr, &ap)) return hipErrorInvalidValue;
    ap.b.items = ws.prune_fail_list;
    ap.n_items_dev = ws.prune_fail_count;
    note_launch(ws.launch_log, wide ? ZSW_LAUNCH_WIDE : ZSW_LAUNCH_V2, Gr, Cr, wide ? (c.mode == 0 ? 0 : 2) : std::min(c.mode, 2));
    pe = wide ? launch_table_cfg_v2_wide(ap, Gr, Cr, c.mode, stream) : launch_table_cfg_v2(ap, Gr, Cr, c.mode, stream);
    if (pe != hipSuccess) return pe;
    hipLaunchKernelGGL(add_count_kernel, dim3(1), dim3(1), 0, stream, ws.prune_fail_count, ws.prune_fail_count + 1);
    return hipGetLastError();
}

// The length classes of a ragged batch: device-side histogram + scatter into ws.bucket_items, counts read back once.
static hipError_t classify_lengths(const ScoreCall& c, BucketCaps* caps, uint32_t counts[NCLS + 1], uint32_t starts[NCLS + 1], hipStream_t stream) {
    const BatchDev& b = c.b;
    const ScoreWorkspace& ws = c.ws;
    for (int k = 0; k < NCLS; ++k) caps->cap[k] = (uint32_t)(kCfgs[kBucketCfg[k]].G * kCfgs[kBucketCfg[k]].C);
    hipError_t e = hipMemsetAsync(ws.bucket_counts, 0, 64 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t hgrid = std::min<uint32_t>(1024, (b.n_items + 255) / 256);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(hgrid), dim3(256), 0, stream, b.offsets, b.n_items, *caps, ws.bucket_counts);
    e = hipMemcpyAsync(counts, ws.bucket_counts, (NCLS + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    uint32_t run = 0;
    for (int k = 0; k <= NCLS; ++k) {
        starts[k] = run;
        run += counts[k];
    }
    e = hipMemcpyAsync(ws.bucket_counts + 32, starts, (NCLS + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bucket_scatter_kernel, dim3(hgrid), dim3(256), 0, stream, b.offsets, b.n_items, *caps, ws.bucket_counts + 32, ws.bucket_items);
    return hipGetLastError();
}

// the items [first, first + n) of ws.bucket_items as a batch
static BatchDev class_items(const ScoreCall& c, uint32_t first, uint32_t n) {
    BatchDev bk = c.b;
    bk.items = c.ws.bucket_items + first;
    bk.n_items = n;
    return bk;
}

// ragged: one launch per occupied length class
static hipError_t score_ragged(ScoreDispatch& d, hipStream_t stream, KernelTimer* timer) {
    const ScoreCall& c = d.call;
    const ScoreWorkspace& ws = c.ws;
    BucketCaps caps;
    uint32_t counts[NCLS + 1], starts[NCLS + 1];
    hipError_t e = classify_lengths(c, &caps, counts, starts, stream);
    if (e != hipSuccess) return e;
    if (timer) timer->begin(stream);
    // The length classes are independent launches and the small ones cannot fill the chip on their own (a class of
    // 70 k reads is two wavefronts per SIMD): they are spread over side streams, forked from and joined to `stream`.
    SideStreams* side = ws.side;  // owned by the context: two contexts never share fork/join events
    const bool fork = side != nullptr && !(ws.debug & ZSW_DEBUG_NO_SIDE_STREAMS);
    if (c.use_v2 && ws.seed && ws.seed_gtab && (ws.debug & ZSW_DEBUG_SCORE_PRUNE) && !(ws.debug & ZSW_DEBUG_PRUNE_STRIP)) {
        // the seeded pass's per-row score table, before the fork: every side stream reads it
        ScoreArgsV2 ag = c.v2, ab = c.v2;
        if (build_tables_v2(c.h_sc, 4, &ag)) {
            e = build_seed_gtabs(d, ag, !(ws.debug & ZSW_DEBUG_SEED_NO_BAND) && doubled_tables(c.h_sc, &ab) ? &ab : nullptr, stream);
            if (e != hipSuccess) return e;
        }
    }
    if (fork) {
        e = hipEventRecord(side->fork, stream);
        if (e != hipSuccess) return e;
        for (int i = 0; i < SideStreams::N; ++i) {
            e = hipStreamWaitEvent(side->s[i], side->fork, 0);
            if (e != hipSuccess) return e;
        }
    }
    int used = 0;  // the classes take the side streams in turn
    // seeded exact pass per length class: each class has its own region of the workspace, its own part of the worklist (at
    // its items' offset) and its own counter, so every class runs its whole pipeline (seed, sort, window, full pass over the
    // reads handed back) on a side stream of its own turn. A handed-back read walks all R rows however few there are of them —
    // 15 ms per class against a 30 kb reference — so these launches must overlap.
    {
        size_t work_off = 0;
        uint32_t n_seedable = 0;  // the banded kernel's blocks are shared among the classes in proportion to their reads
        for (int k = 0; k < NCLS; ++k) n_seedable += counts[k];
        for (int k = NCLS - 1; k >= 0; --k) {
            if (!counts[k]) continue;
            const Cfg& cf = kCfgs[kBucketCfg[k]];
            const uint32_t grid_cap = seed_band_class_cap(counts[k], n_seedable);
            e = seed_items(d, class_items(c, starts[k], counts[k]), cf.G, cf.C, caps.cap[k], work_off, starts[k], ws.prune_fail_count + 2 + k, grid_cap,
                           nullptr, fork ? side->s[used % SideStreams::N] : stream);
            if (e == hipSuccess) {
                ++used;
                work_off += seed_workspace_bytes(counts[k], caps.cap[k], grid_cap);
                counts[k] = 0;
            } else if (e != hipErrorNotSupported) {
                return e;
            }
        }
    }
    // column-pruned pass (strip + window; ZSW_DEBUG_PRUNE_STRIP): consecutive length classes that share a pruning class form
    // one item range, and pruning classes with the same strip width share the strip launch
    {
        int k0[PR_N_CLASSES], k1[PR_N_CLASSES];
        uint32_t cnt[PR_N_CLASSES];
        for (int pc = 0; pc < PR_N_CLASSES; ++pc) {
            k0[pc] = k1[pc] = -1;
            cnt[pc] = 0;
            for (int k = 0; k < NCLS; ++k) {
                const uint32_t cap = caps.cap[k];
                if (cap <= kPruneClasses[pc].max_len && (pc == 0 || cap > kPruneClasses[pc - 1].max_len) && cap > (uint32_t)kPruneClasses[pc].cp + 40) {
                    if (k0[pc] < 0) k0[pc] = k;
                    k1[pc] = k;
                    cnt[pc] += counts[k];
                }
            }
        }
        for (int pc = 0; pc < PR_N_CLASSES; ++pc) {
            if (k0[pc] < 0) continue;
            int last = pc;
            if (pc + 1 < PR_N_CLASSES && k0[pc + 1] == k1[pc] + 1 && kPruneClasses[pc + 1].cp == kPruneClasses[pc].cp && c.ref_len < (1u << 24)) last = pc + 1;
            const BatchDev bp = class_items(c, starts[k0[pc]], starts[k1[last]] + counts[k1[last]] - starts[k0[pc]]);
            if (bp.n_items) {
                e = prune_items(c, bp, pc, cnt[pc], stream);
                if (e == hipSuccess) {
                    for (int k = k0[pc]; k <= k1[last]; ++k) counts[k] = 0;
                } else if (e != hipErrorNotSupported) {
                    return e;
                }
            }
            pc = last;
        }
    }
    for (int k = NCLS; k >= 0; --k) {  // longest class first
        if (!counts[k]) continue;
        const BatchDev bk = class_items(c, starts[k], counts[k]);
        if (k == NCLS) {  // longer than every strip configuration; stays on the main stream (shares scratch with the pass below)
            e = launch_tiled(c, bk, c.max_len, stream);
            if (e == hipErrorNotSupported) e = launch_exact32(c, bk, nullptr, nullptr, nullptr, nullptr, stream);
        } else {
            e = launch_one(c, bk, kCfgs[kBucketCfg[k]].G, kCfgs[kBucketCfg[k]].C, fork ? side->s[used++ % SideStreams::N] : stream);
        }
        if (e != hipSuccess) return e;
    }
    if (fork) {
        for (int i = 0; i < SideStreams::N; ++i) {
            e = hipEventRecord(side->join[i], side->s[i]);
            if (e != hipSuccess) return e;
            e = hipStreamWaitEvent(stream, side->join[i], 0);
            if (e != hipSuccess) return e;
        }
    }
    if (timer) timer->end(stream);
    return hipSuccess;
}

static hipError_t launch_score_passes(const ScoringDev* d_sc, const ScoringDev& h_sc, const BatchDev& b, uint32_t max_len,
                                      const uint8_t* d_ref, uint32_t ref_len, const ResultRule& rule, const ScoreOut& out,
                                      const ScoreWorkspace& ws, hipStream_t stream, KernelTimer* timer, int mode) {
    hipError_t e = hipMemsetAsync(out.fb_count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    ScoreDispatch d{ScoreCall(d_sc, h_sc, b, max_len, d_ref, ref_len, rule, out, ws, mode)};
    const ScoreCall& c = d.call;
    int G = 0, C = 0;
    if (!c.table_ok) {  // alphabet outside the table kernels: exact kernel over the whole batch
        if (timer) timer->begin(stream);
        e = launch_exact32(c, b, nullptr, nullptr, nullptr, nullptr, stream);
        if (timer) timer->end(stream);
        return e;
    }
    if (b.offsets && !b.items && b.n_items > 0) {
        e = score_ragged(d, stream, timer);
    } else if (!score_config_for_batch(max_len, b.n_items, &G, &C)) {  // longer than every strip configuration
        if (timer) timer->begin(stream);
        BatchDev bl = b;
        if (!bl.items && ws.bucket_items) {  // the tiles address reads through an item list
            hipLaunchKernelGGL(iota_kernel, dim3((b.n_items + 255) / 256), dim3(256), 0, stream, ws.bucket_items, b.n_items);
            bl.items = ws.bucket_items;
        }
        e = launch_tiled(c, bl, max_len, stream);
        const bool tiled = e != hipErrorNotSupported;
        if (!tiled) e = launch_exact32(c, b, nullptr, nullptr, nullptr, nullptr, stream);
        if (timer) timer->end(stream);
        if (!tiled) return e;
    } else {
        // The seeded exact pass (zsw_score_seed.hip), or the column-pruned pass (zsw_score_prune.hip; ZSW_DEBUG_PRUNE_STRIP); the
        // reads they hand back are scored over all their cells. Otherwise the full pass. One timed interval either way.
        if (timer) timer->begin(stream);
        e = hipErrorNotSupported;
        int Gs = 0, Cs = 0;
        if (score_config_for(max_len, &Gs, &Cs)) e = seed_items(d, b, Gs, Cs, max_len, 0, 0, ws.prune_fail_count, SEED_BAND_MAX_GRID, ws.side, stream);
        const int cls = prune_class_for(max_len);
        if (e == hipErrorNotSupported && cls >= 0) e = prune_items(c, b, cls, b.n_items, stream);
        if (e == hipErrorNotSupported) e = launch_one(c, b, G, C, stream);
        if (timer) timer->end(stream);
    }
    if (e != hipSuccess) return e;
    return finish_worklist(c, stream);
}

hipError_t launch_score(const ScoringDev* d_sc, const ScoringDev& h_sc, const BatchDev& b, uint32_t max_len,
                        const uint8_t* d_ref, uint32_t ref_len, const ResultRule& rule, const ScoreOut& out,
                        const ScoreWorkspace& ws, hipStream_t stream, KernelTimer* timer, int mode) {
    hipError_t e = launch_score_passes(d_sc, h_sc, b, max_len, d_ref, ref_len, rule, out, ws, stream, timer, mode);
    if (e != hipSuccess || !ws.min_score || !ws.min_counts || b.n_items == 0) return e;
    hipLaunchKernelGGL(min_filter_kernel, dim3(std::min<uint32_t>((b.n_items + 255) / 256, 4096u)), dim3(256), 0, stream, b, min_threshold(rule, ws.min_score), out,
                       ws.min_counts + 2);
    return hipGetLastError();
}

// ---- reverse pass of sw_simd_score_ranges -------------------------------------------------------------------
__global__ void gtab_kernel(const uint8_t* ref, uint32_t n, const ScoringDev* sc, ScoreArgs a, int wide, uint2* gtab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int idx = sc->index_map[ref[i]];
        gtab[i] = wide ? make_uint2((uint32_t)(idx * WIDE_STRIDE), 0u) : make_uint2(a.wtab[idx][0], a.wtab[idx][1]);
    }
}

template <int G, int C>
static hipError_t launch_cfg_rev(const ScoreArgs& a, bool fast, hipStream_t stream) {
    const uint32_t reads_per_block = 2 * (BLOCK / G);
    const uint32_t grid = (a.b.n_items + reads_per_block - 1) / reads_per_block;
    if (grid == 0) return hipSuccess;
    if (fast) hipLaunchKernelGGL((score_kernel<G, C, true, 2, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    else hipLaunchKernelGGL((score_kernel<G, C, false, 2, true>), dim3(grid), dim3(BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_score_rev(const ScoringDev* d_sc, const ScoringDev& h_sc, const BatchDev& b, uint32_t max_len,
                            const uint8_t* d_ref, uint32_t ref_len, const ResultRule& rule, const ScoreOut& out,
                            const ScoreWorkspace& ws, const uint32_t* d_fwd_ref_end, const uint32_t* d_fwd_query_end,
                            const uint32_t* d_fwd_score, uint2* d_gtab, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out.fb_count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const ScoreCall c(d_sc, h_sc, b, max_len, d_ref, ref_len, rule, out, ws, 2);
    int G = 0, C = 0;
    const bool fits = score_config_for(max_len, &G, &C);
    if (!fits && ws.tile_buf && ws.tile_state && ws.bucket_items && w32_ok(h_sc, ref_len, max_len, ws.debug) && b.n_items) {
        // reads longer than every strip configuration: the 32-bit tile kernel over the reversed reference (held in d_gtab's bytes)
        uint8_t* d_rev = reinterpret_cast<uint8_t*>(d_gtab);
        if (ref_len) hipLaunchKernelGGL(reverse_bytes_kernel, dim3((ref_len + 255) / 256), dim3(256), 0, stream, d_ref, ref_len, d_rev);
        hipLaunchKernelGGL(iota_kernel, dim3((b.n_items + 255) / 256), dim3(256), 0, stream, ws.bucket_items, b.n_items);
        ScoreArgsV2 a2 = w32_args(c);
        a2.ref = d_rev;
        a2.rev_ref_end = d_fwd_ref_end;
        a2.rev_query_end = d_fwd_query_end;
        const uint32_t per_round = tile_round_items(c, 1, b.n_items);
        if (per_round)
            return tile_rounds(c, a2, b.n_items, per_round, max_len, ZSW_LAUNCH_TILE_W32,
                               [&](const ScoreArgsV2& a, uint32_t first) { return launch_tile_w32(a, ws.bucket_items + first, 2, stream); });
    }
    if (!c.table_ok || !fits) return launch_exact32(c, b, nullptr, nullptr, d_fwd_ref_end, d_fwd_query_end, stream);
    ScoreArgs a = c.v1;  // (not WIDE: with build_tables' tables)
    a.rev_ref_end = d_fwd_ref_end;
    a.rev_query_end = d_fwd_query_end;
    a.rev_score = d_fwd_score;
    a.gtab = d_gtab;
    if (c.wide) {
        for (int r = 0; r < 33; ++r)
            for (int q = 0; q < WIDE_STRIDE; ++q)
                a.wide[r * WIDE_STRIDE + q] = (int8_t)((r < h_sc.S && q < h_sc.S) ? h_sc.w[r * h_sc.S + q] : 0);
        a.go2 = ((uint32_t)h_sc.gap_open & 0xffffu) * 0x00010001u;
        a.ge2 = ((uint32_t)h_sc.gap_extend & 0xffffu) * 0x00010001u;
        a.bias2 = 0;
    }
    if (ref_len) hipLaunchKernelGGL(gtab_kernel, dim3((ref_len + 255) / 256), dim3(256), 0, stream, d_ref, ref_len, d_sc, a, (int)c.wide, d_gtab);
    if (b.n_items) note_launch(ws.launch_log, c.wide ? ZSW_LAUNCH_WIDE_REV : c.fast ? ZSW_LAUNCH_V1_FAST_REV : ZSW_LAUNCH_V1_BIASED_REV, G, C, 2);
    if (c.wide) {
        e = launch_cfg_rev_wide(a, G, C, stream);
    } else {
        switch (G * 100 + C) {
#define ZSW_CASE(GV, CV) \
    case GV * 100 + CV: e = launch_cfg_rev<GV, CV>(a, c.fast, stream); break;
            ZSW_FOR_EACH_STRIP_CONFIG(ZSW_CASE)
#undef ZSW_CASE
            default: e = hipErrorInvalidValue;
        }
    }
    if (e != hipSuccess) return e;
    return launch_exact32(c, b, out.fb_list, out.fb_count, d_fwd_ref_end, d_fwd_query_end, stream);
}

}  // namespace zsw
