// zsw_context.hpp — the context behind the C ABI and the helpers its translation units share (zsw_capi.hip: the entry points
// with the read as the profile; zsw_capi_shared.hip: the one-profile-many-sequences role; the staging tables of a host call's
// arrays and the overlap checks of the record and text calls). Not installed.
#pragma once
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "zsw_align.hpp"
#include "zsw_internal.hpp"
#include "zsw_score_prune.hpp"
#include "zsw_score_seed.hpp"
#include "zsw_shared.hpp"
#include "zsw_timer.hpp"

namespace zsw {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() { return reinterpret_cast<T*>(p); }
};

struct Panel;  // zsw_panel.hpp

}  // namespace zsw

struct zsw_context {
    int device = 0;
    uint32_t cu_count = 256;
    bool scoring_set = false, reference_set = false;
    zsw::ScoringDev h_sc{};
    zsw::ScoringDev h_sc_t{};  // h_sc with the matrix transposed (d_sc_t on the device): the shared-profile role's role-swapped passes
    int bias = 0;
    zsw::DevBuf d_sc, d_ref, d_fb_list, d_fb_count, d_scratch, d_maxlen, d_bucket_items, d_bucket_counts, d_tile_buf, d_tile_state;
    zsw::DevBuf d_prune, d_prune_list, d_prune_count;  // column-pruned score pass; the worklist and its counters also serve the seeded pass
    // seeded exact score pass (zsw_score_seed.hip): index of the reference under the current matrix (built with the first batch
    // that can use it, rebuilt after zsw_set_scoring / zsw_set_reference), a host copy of the reference to build it from
    zsw::SeedIndex seed;
    // the same for the REVERSED reference (d_ref_rev): the reverse pass of sw_simd_score_ranges as a second seeded pass over the
    // reversed reads (zsw_capi.hip, ranges_device); built with the first such call
    zsw::SeedIndex seed_rev;
    zsw::DevBuf d_ref_rev;
    std::vector<uint8_t> h_ref;
    zsw::DevBuf d_seed_work, d_seed_gtab, d_chunk_keys;
    size_t ref_len = 0;
    uint32_t scratch_len = 0;
    size_t exact_slots = 0;
    // staging for host-memory batches
    zsw::DevBuf s_bases, s_packed, s_offsets, s_score, s_status, s_tier, s_rend, s_qend;
    // alignment workspace (zsw_align.hip)
    zsw::DevBuf a_ws[30];
    // score_ranges workspace
    zsw::DevBuf r_ws[24];
    zsw::KernelTimer timer;
    zsw::KernelTimer timer_window;  // seed_window_kernel launches alone
    std::string err;
    uint32_t debug = 0;    // zsw_debug_set (kernel-selection overrides for tests)
    int32_t* band_dbg = nullptr;  // zsw_debug_band_records (tests: the banded seeded pass reports the values it decides with)
    int32_t* cert_dbg = nullptr;  // zsw_debug_cert_records (tests: the certificate pass reports its verdict per read)
    int32_t* tp_dbg = nullptr;    // zsw_debug_threepass_records (tests: the third pass of the 3-pass calls reports each read's route)
    std::vector<uint32_t> score_launches;  // zsw_debug_score_launches (tests: the score kernels the last call launched, 4 entries each)
    uint32_t options = ZSW_DEBUG_SCORE_PRUNE;  // zsw_set_option, as ZSW_DEBUG_* bits; exact pruning is on by default
    uint32_t flags() const { return debug | options; }
    // ZSW_OPTION_MIN_SCORE: T (0 = off), and three device counters of the last covered call (ScoreWorkspace::min_counts), zeroed
    // by stage() while the option is on
    uint32_t min_score = 0;
    zsw::DevBuf d_min_counts;
    // What zsw_prune_rescored and zsw_min_score_counts report on: the last call that stage() planned (written there once its plan is
    // complete; a call rejected before that leaves the record of the call before it). The only per-call state the context keeps:
    // everything else about a call travels in its Staged value.
    struct LastCall {
        bool handbacks_counted = false;  // d_prune_count[1] counts this call's hand-backs (it took the seeded or the column-pruned pass)
        bool min_counts_valid = false;   // d_min_counts holds this call's counters (zsw_set_option(MIN_SCORE, 0) clears it)
    } last;
    // host batches: reads of chunk k+1 cross PCIe on this stream while chunk k computes
    hipStream_t copy_stream = nullptr;
    std::vector<hipEvent_t> copy_events;
    // ragged batches: the length classes run on these (created with the first ragged batch)
    zsw::SideStreams* side = nullptr;
    // the one-profile-many-sequences role (zsw_capi_shared.hip): the sequence the shared profile is built from, the scoring with
    // the matrix transposed (score-only calls go through the ordinary kernels with the roles swapped), workspace
    zsw::DevBuf d_pseq, d_pseq_rev, d_sc_t, sh_ws[20];
    std::vector<uint8_t> h_pseq;
    size_t pseq_len = 0;
    bool pseq_set = false;
    // index of the profile sequence under the transposed matrix: the seeded pass of the shared role's score calls (roles swapped:
    // the sequence is the ordinary kernels' reference); rebuilt after zsw_set_scoring / zsw_set_profile_sequence
    zsw::SeedIndex seed_shared;
    // the same for the REVERSED profile sequence (d_pseq_rev): the second pass of the shared role's sw_simd_score_ranges as a
    // seeded pass over the reversed reads (zsw_capi_shared.hip, run_ranges_shared); built with the first such call
    zsw::SeedIndex seed_shared_rev;
    // strand-aware calls (zsw_strand.hip): the complement table (empty = the IUPAC default), workspace — the staged batch of a host
    // call, the oriented copy, the second batch of the reads scored on both strands and its results, 8 bytes per read of what the
    // seed kernel found, the list of unsettled reads and the counters of zsw_strand_counts — and the host copy a host batch is
    // oriented into for the 3-pass call
    std::vector<uint8_t> complement;
    zsw::DevBuf st_ws[24];
    std::vector<uint8_t> h_orient;
    int32_t* strand_dbg = nullptr;  // zsw_debug_strand_records
    // reference panels (zsw_panel.hip, zsw_panel.hpp): the members of zsw_set_panel with an index each, the workspace of the panel
    // calls and the counters of the last one; null until zsw_set_panel
    zsw::Panel* panel = nullptr;
    int32_t* panel_dbg = nullptr;  // zsw_debug_panel_records
    // zsw_annotate_batch (zsw_annotate.hip): the staged arrays of a host call, the verbose ciglet counts and their exclusive sum
    zsw::DevBuf an_ws[16];
    // zsw_sam_batch (zsw_sam.hip): the staged arrays of a host call, RNAME, the line lengths / starts, the lines' shapes, the text
    zsw::DevBuf sam_ws[20];
    // zsw_pileup_batch / zsw_consensus_from_counts (zsw_pileup.hip): the accumulators (16 bytes per site), the scan's scratch, the
    // counter of malformed records, the staged arrays and tables of a host call
    zsw::DevBuf pu_ws[16];
    // the newline (for FASTA: '>') index of the parse calls (zsw_text.hip): the staged text of a host call, the tile counts and their sum, 8 bytes
    // per newline. One set for all of them: the context keeps the larger workspace
    zsw::DevBuf text_ws[4];
    // zsw_fastq_parse_batch (zsw_fastq.hip): the per-record arrays and their sums, the scans' scratch, the state block with the
    // report, the staged outputs of a host call
    zsw::DevBuf fq_ws[12];
    // zsw_sam_parse_batch (zsw_samtext.hip): 120 bytes and six sums per line, the scans' scratch, the state block with the report,
    // RNAME, the staged outputs of a host call
    zsw::DevBuf samtext_ws[24];
    // zsw_fasta_parse_batch (zsw_fasta.hip): 25 bytes and one sum per '>', 16 bytes per tile for the kept bytes, the scans' scratch,
    // the state block with the report, the staged outputs of a host call. The '>' index uses text_ws
    zsw::DevBuf fa_ws[14];
};

namespace zsw {
namespace capi {

constexpr size_t EXACT_SLOTS = 64 * 256;               // rows of the exact 32-bit kernel that run at once, at most
constexpr size_t EXACT_SCRATCH_BUDGET = size_t(1) << 30;  // bytes of its H/E rows, at most (longer reads get fewer slots)
constexpr uint32_t LONGEST_STRIP = 64 * 38;  // columns of the widest strip configuration (zsw_score_v2.hpp)

inline zsw_error fail(zsw_context* ctx, zsw_error code, const char* what, hipError_t e = hipSuccess) {
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) {
            ctx->err += ": ";
            ctx->err += hipGetErrorString(e);
        }
    }
    return code;
}

// Makes the context's GPU current for the duration of a public call and puts the caller's device back afterwards: a
// single-process multi-GPU host (zsw_group, or PyTorch with several devices) must not find its current device changed.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const zsw_context* ctx) {
        if (!ctx) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != ctx->device) (void)hipSetDevice(ctx->device);
        else prev = -1;  // nothing to restore
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define ZSW_HIP(ctx, call)                                                     \
    do {                                                                       \
        hipError_t _e = (call);                                                \
        if (_e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, #call, _e);        \
    } while (0)

// ---- host calls: staging by table -------------------------------------------------------------------------------------------
// An input array of a host call: `bytes` at `src` go to ws[slot], and *dev points there. An absent array (src == nullptr) stays
// absent; an array of zero bytes gets its place and no copy.
struct Up {
    int slot;
    const void* src;
    size_t bytes;
    const void** dev;
};
inline zsw_error stage_up(zsw_context* ctx, DevBuf* ws, const Up* ups, int n, hipStream_t stream) {
    for (const Up* u = ups; u < ups + n; ++u) {
        if (!u->src) continue;
        ZSW_HIP(ctx, ws[u->slot].ensure(u->bytes + 16));
        if (u->bytes) ZSW_HIP(ctx, hipMemcpyAsync(ws[u->slot].p, u->src, u->bytes, hipMemcpyHostToDevice, stream));
        *u->dev = ws[u->slot].p;
    }
    return ZSW_OK;
}
// The six arrays every alignment call returns, as the kernels' arguments hold them (a->bases, offsets, aln, status, inc, op; a->n,
// a->n_ciglets), to ws[0 .. 5]. bases: null = not wanted on the device.
template <class Args>
zsw_error stage_up_records(zsw_context* ctx, DevBuf* ws, const uint8_t* bases, size_t base_bytes, Args* a, hipStream_t stream) {
    const size_t n = a->n;
    const Up ups[6] = {{0, bases, base_bytes, (const void**)&a->bases},           {1, a->offsets, (n + 1) * 8, (const void**)&a->offsets},
                       {2, a->aln, n * sizeof(zsw_alignment), (const void**)&a->aln}, {3, a->status, n, (const void**)&a->status},
                       {4, a->inc, (size_t)a->n_ciglets * 4, (const void**)&a->inc},  {5, a->op, (size_t)a->n_ciglets, (const void**)&a->op}};
    return stage_up(ctx, ws, ups, 6, stream);
}
// An output array of a host call: before the launches *dev (the caller's array; absent stays absent) is redirected to ws[slot] with
// room for `bytes`; after them copy_down() copies what was used to the caller's array (nothing for zero bytes).
struct Down {
    int slot;
    size_t bytes;
    void** dev;
    void* dst;  // set by stage_down
};
inline zsw_error stage_down(zsw_context* ctx, DevBuf* ws, Down* downs, int n) {
    for (Down* d = downs; d < downs + n; ++d) {
        d->dst = *d->dev;
        if (!d->dst) continue;
        ZSW_HIP(ctx, ws[d->slot].ensure(d->bytes + 16));
        *d->dev = ws[d->slot].p;
    }
    return ZSW_OK;
}
inline zsw_error copy_down(zsw_context* ctx, const Down* downs, const size_t* used, int n, hipStream_t stream) {
    for (int k = 0; k < n; ++k)
        if (downs[k].dst && used[k]) ZSW_HIP(ctx, hipMemcpyAsync(downs[k].dst, *downs[k].dev, used[k], hipMemcpyDeviceToHost, stream));
    return ZSW_OK;
}

// do [a, a + na) and [b, b + nb) share a byte? An absent or empty array overlaps nothing
inline bool overlaps(const void* a, uint64_t na, const void* b, uint64_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
struct Span {
    const void* p;
    uint64_t bytes;
};
// the lowest i for which s[i] overlaps a later span; -1: none does
inline int first_overlap(const Span* s, int n) {
    for (int i = 0; i < n; ++i)
        for (int k = i + 1; k < n; ++k)
            if (overlaps(s[i].p, s[i].bytes, s[k].p, s[k].bytes)) return i;
    return -1;
}

inline bool valid_lanes(int lanes) { return lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64; }

inline uint64_t signed_thr(int bits) { return bits == 8 ? 255ull : bits == 16 ? 65535ull : 4294967295ull; }

// The arguments of a public call with one <T, N>: its result rule, or the error the call returns.
// score_to_maybe_aligned (striped.rs:610-633) as a threshold on the true score:
//   signed T  : Overflowed  <=>  best >= T::MAX            <=>  s >= 2^bits - 1
//   unsigned T: Overflowed  <=>  best + bias + 1 > T::MAX  <=>  s >= T::MAX - bias
inline zsw_error rule_direct(zsw_context* ctx, zsw_int_type t, int lanes, ResultRule* r) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (!valid_lanes(lanes)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "lanes must be a power of two in 2..64");
    const int bias = ctx->bias;
    r->n_tiers = 1;
    switch (t) {
        case ZSW_I8: r->thr[0] = signed_thr(8); r->tier_code[0] = 8; return ZSW_OK;
        case ZSW_I16: r->thr[0] = signed_thr(16); r->tier_code[0] = 16; return ZSW_OK;
        case ZSW_I32: r->thr[0] = signed_thr(32); r->tier_code[0] = 32; return ZSW_OK;
        case ZSW_U8:
            r->thr[0] = 255ull - (uint64_t)bias;
            r->tier_code[0] = 8;
            if (bias < 255) return ZSW_OK;
            break;
        case ZSW_U16: r->thr[0] = 65535ull - (uint64_t)bias; r->tier_code[0] = 16; return ZSW_OK;
        case ZSW_U32: r->thr[0] = 4294967295ull - (uint64_t)bias; r->tier_code[0] = 32; return ZSW_OK;
    }
    return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "bad int_type");
}

// The arguments of a public _from call: the or_else_overflowed chain (profile_set.rs:71-107), i8 -> i16 -> i32 from `from_width`
inline zsw_error rule_cascade(zsw_context* ctx, int from_width, int preset_bits, ResultRule* r) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (preset_bits != 128 && preset_bits != 256 && preset_bits != 512) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "preset_bits");
    if (from_width != 8 && from_width != 16 && from_width != 32) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "from_width");
    r->n_tiers = 0;
    for (int w = from_width; w <= 32; w *= 2) {
        r->thr[r->n_tiers] = signed_thr(w);
        r->tier_code[r->n_tiers] = (uint8_t)w;
        ++r->n_tiers;
    }
    return ZSW_OK;
}

// Entry points ZSW_OPTION_MIN_SCORE does not cover refuse to run while it is set (and write nothing)
inline zsw_error min_score_unsupported(zsw_context* ctx, const char* what) {
    if (!ctx || !ctx->min_score) return ZSW_OK;
    ctx->err = std::string(what) + ": not covered by ZSW_OPTION_MIN_SCORE; set the option to 0 for this call";
    return ZSW_ERR_UNSUPPORTED;
}

// are the n + 1 offsets of a host batch in ascending order? *longest (optional): the longest read
inline bool offsets_monotone(const uint64_t* offsets, uint64_t n, uint32_t* longest = nullptr) {
    uint32_t m = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return false;
        m = std::max<uint32_t>(m, (uint32_t)(offsets[i + 1] - offsets[i]));
    }
    if (longest) *longest = m;
    return true;
}

// How a call is put together: target -> stage -> plan -> run -> deliver. The entry point names what the reads are scored against
// (Against) and where the results go (ScoreDest / AlignDest / RangesDev); stage() brings the batch to the device and decides the
// passes the batch takes (CallPlan, inside Staged); the run_* functions launch from the Staged value; unstage() / copy_ranges_out() /
// finish_alignments() deliver. stage() is a function of its arguments and of the context's configuration and buffers: what stays on
// the context between calls is the growing buffers, the lazily built indices and the last-call record (zsw_context::last).

// The target of a call: what the ordinary score kernels treat as their reference, the scoring that goes with it, the index that
// serves its seeded pass.
struct Against {
    const uint8_t* d_seq;  // the sequence on the device, and the host copy the index is built from
    const uint8_t* h_seq;
    size_t len;
    const ScoringDev *d_sc, *h_sc;
    SeedIndex* index;
    bool set;        // the sequence has been given
    bool may_prune;  // the column-pruned pass may run
};
// the read-as-profile role: the reads against the context's reference
inline Against against_reference(zsw_context* c) {
    if (!c) return Against{};
    return Against{c->d_ref.as<uint8_t>(), c->h_ref.data(), c->ref_len, c->d_sc.as<ScoringDev>(), &c->h_sc, &c->seed, c->reference_set, true};
}
// the shared role's score passes swap the roles: the profile sequence is the ordinary kernels' reference, the matrix transposed
inline Against against_profile_sequence(zsw_context* c) {
    if (!c) return Against{};
    return Against{c->d_pseq.as<uint8_t>(), c->h_pseq.data(), c->pseq_len, c->d_sc_t.as<ScoringDev>(), &c->h_sc_t, &c->seed_shared, c->pseq_set, false};
}

// The result arrays of a score call (tier, ref_end, query_end: null = not wanted), and of an alignment call (tier: null = not wanted)
struct ScoreDest {
    uint32_t* score;
    uint8_t *status, *tier;
    uint32_t *ref_end, *query_end;
    bool ends() const { return ref_end && query_end; }
};
struct AlignDest {
    zsw_alignment* aln;
    uint8_t *status, *tier;
    uint32_t* inc;
    uint8_t* op;
    uint64_t ciglet_cap;
    uint64_t* n_ciglets;
};

// The passes stage() decided this call's batch takes
struct CallPlan {
    SeedIndex* seed = nullptr;  // the seeded pass runs with this index (workspace and worklist are in place); null: no seeded pass
    bool chunk_keys = false;    // ... and d_chunk_keys holds a key per read (long references: the hand-back pass runs in chunks of rows)
    uint32_t prune_chunk = 0;   // reads per round of the column-pruned pass; 0: it does not run
    bool min_counts = false;    // ZSW_OPTION_MIN_SCORE is on: d_min_counts was zeroed for this call
};

struct Staged {
    BatchDev b{};
    uint32_t max_len = 0;
    // where the kernels write the results: the caller's arrays (device batch) or the staging buffers (host batch); all null for a
    // call whose results stay in library workspace
    ScoreDest dev{};
    CallPlan plan{};
};

// a ScoreOut over `d` with the context's fall-back list
inline ScoreOut score_out(zsw_context* ctx, const ScoreDest& d) {
    ScoreOut o;
    o.score = d.score;
    o.status = d.status;
    o.tier = d.tier;
    o.ref_end = d.ref_end;
    o.query_end = d.query_end;
    o.fb_list = ctx->d_fb_list.as<uint32_t>();
    o.fb_count = ctx->d_fb_count.as<uint32_t>();
    return o;
}

// zsw_capi.hip: the bodies of zsw_score_batch(_from) and zsw_align_3pass_batch(_from), which the strand-aware calls run on oriented
// batches and the panel call on the groups of a batch, each against its member (`target`)
zsw_error run_score(zsw_context* ctx, const Against& target, const zsw_batch* reads, const ResultRule& rule, const ScoreDest& dest, void* stream);
// zsw_panel.hip: the context's panel after zsw_set_scoring (its indices spell k-mers with the matrix's good residues), in zsw_destroy
void panel_invalidate(zsw_context* ctx);
void panel_release(zsw_context* ctx);
zsw_error run_threepass(zsw_context* ctx, const zsw_batch* reads, const ResultRule& rule, int invert, const AlignDest& dest, void* stream);
// zsw_capi.hip. dest: null = the results stay in library workspace (ranges, alignments): no staging of score / status
zsw_error stage(zsw_context* ctx, const Against& target, const zsw_batch* reads, const ScoreDest* dest, hipStream_t stream, Staged* st,
                bool defer_bases_copy = false);
// prologue of the alignment calls: null checks, stage(), *dest.n_ciglets = 0 (the caller returns at once for an empty batch)
zsw_error stage_align(zsw_context* ctx, const Against& target, const zsw_batch* reads, const AlignDest& dest, hipStream_t stream, Staged* st);
ScoreWorkspace score_ws(zsw_context* ctx, const Staged& st);
zsw_error unstage(zsw_context* ctx, const zsw_batch* reads, hipStream_t stream, const Staged& st, const ScoreDest& dest);
enum { WS_SCORE = 0, WS_STATUS, WS_TIER, WS_REND, WS_ITEMS, WS_RING, WS_CIG, WS_ALN, WS_CIGSTART, WS_CIGRAW, WS_BSUMS, WS_TOTAL,
       WS_FBLIST, WS_FBCOUNT, WS_OINC, WS_OOP, WS_CIG2, WS_RING2, WS_KEYS_IN, WS_KEYS_OUT, WS_VALS_IN, WS_SORT_TMP, WS_GTABLE, WS_FBMETA,
       WS_ITEMS2, WS_SAFE, WS_CERT_OK, WS_CERT_DONE, WS_CERT_STATUS };
enum { RW_FSCORE = 0, RW_FSTATUS, RW_FREND, RW_FQEND, RW_RSCORE, RW_RSTATUS, RW_RRS, RW_RQS, RW_QEM, RW_GTAB, RW_MIS, RW_O0, RW_O1,
       RW_O2, RW_O3, RW_O4, RW_O5, RW_FTIER, RW_UNIQ_F, RW_UNIQ_R, RW_RBASES, RW_ULIST, RW_UCOUNT };
zsw_error finish_alignments(zsw_context* ctx, DevBuf* ws, uint32_t n, bool host, const uint8_t* d_status, const uint8_t* d_tier, int invert,
                            const AlignDest& dest, hipStream_t stream);
struct RangesDev {  // the arrays of sw_simd_score_ranges for every read: library workspace on the device, or the caller's (tier: may be null)
    uint32_t *score, *rs, *re, *qs, *qe;
    uint8_t *status, *tier;
};
// the ranges to the caller's arrays (a host batch: the call returns once they are there)
zsw_error copy_ranges_out(zsw_context* ctx, const RangesDev& rd, uint32_t n, bool host, const RangesDev& out, hipStream_t stream);
// the seed index of a reversed sequence (`seq` back to front, uploaded to `d_rev`) under `sc`, unless it is valid already
zsw_error reversed_seed_index(zsw_context* ctx, SeedIndex* index, DevBuf* d_rev, const std::vector<uint8_t>& seq, const ScoringDev& sc, hipStream_t stream);
// sw_align_3pass's third pass (zsw_threepass.hip) over ranges that are already on the device, results to the caller's arrays; the
// caller has opened ctx->timer's interval. pseq: non-null = the shared-profile role (ThreePassArgs::pseq).
zsw_error threepass_third_pass(zsw_context* ctx, const Staged& st, const RangesDev& rd, const uint8_t* pseq, uint32_t pseq_len, bool host, int invert,
                               const AlignDest& dest, hipStream_t stream);
// The certificate pass of sw_simd_align in both roles (tests/models/align_gapless_cert.cpp, align_onegap_cert.cpp): the classify
// launches of zsw_threepass.hip write the alignment of every read of `rd` they can certify (settled[i]: both maxima of read i sit in
// one cell each). *pass2_status: the statuses the literal second pass sees — a certified read does not take part. pseq: as above.
zsw_error certificate_pass(zsw_context* ctx, const Staged& st, const RangesDev& rd, const uint8_t* settled, const uint8_t* pseq, uint32_t pseq_len,
                           int invert, hipStream_t stream, const uint8_t** pass2_status);
// zsw_capi_shared.hip: the settlement of a reversed seeded pass (a read is
// done if both maxima sit in one cell each and the scores agree; the others are listed for the exact reverse kernel)
hipError_t launch_settle_reverse(const BatchDev& b, uint32_t n, uint32_t other_len, const uint8_t* uf, const uint8_t* ur, const uint32_t* fscore,
                                 const uint8_t* fstatus, const uint32_t* rscore, const uint8_t* rstatus, uint32_t* read_side, uint32_t* other_side,
                                 uint32_t* list, uint32_t* count, hipStream_t stream, uint8_t* settled = nullptr);  // settled[i] = 1: read i is done
// the and_then / map chain of sw_simd_score_ranges on device arrays (kernels of zsw_capi.hip)
hipError_t launch_ranges_prep(uint32_t n, const uint8_t* fstatus, const uint32_t* fqend, uint32_t* qe_masked, hipStream_t stream);
hipError_t launch_ranges_combine(uint32_t n, const uint32_t* fscore, const uint8_t* fstatus, const uint32_t* frend, const uint32_t* fqend,
                                 const uint32_t* rscore, const uint8_t* rstatus, const uint32_t* rrstart, const uint32_t* rqstart,
                                 uint32_t* out_score, uint32_t* out_rs, uint32_t* out_re, uint32_t* out_qs, uint32_t* out_qe,
                                 uint8_t* out_status, uint32_t* mismatch, hipStream_t stream);

}  // namespace capi
}  // namespace zsw
