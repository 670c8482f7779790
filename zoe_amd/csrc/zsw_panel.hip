// zsw_panel.hip — reference panels (include/zoe_sw.h: zsw_set_panel, zsw_score_panel_batch_from, zsw_panel_gather_batch,
// zsw_panel_counts). The contract: R_k = f(read) with member k of the panel as the reference, f = zsw_score_batch_from; the answer is
// R_k of the member that ranks highest (OVERFLOWED > SOME by score > UNMAPPED = EMPTY), ties to the lowest k, bit for bit what f
// returns against that member.
//
// Scoring every read against every member is n_refs full-price calls, in each of which the reads of the other members have no
// anchor and cost every cell. Instead, per read:
//   1  panel_seed_kernel sweeps the read under each member's SeedParams (zsw_seed.hpp: seed_whole_sweep), looks the sampled k-mers
//      up in that member's index and keeps the first choice p — the member with the largest support of the anchor vote, ties to the
//      lowest — and, per member, claim W's bound U_k: no local alignment of the read against member k scores more than U_k;
//   2  first round: the reads are grouped by p, each group is written as a compact batch and scored by the existing score pass with
//      member p as its target; the results go back by read id;
//   3  panel_settle_kernel: with S the score against p (status SOME), member k != p is ruled out iff U_k < S, or U_k = S and k > p
//      (seed_panel_ruled_out); every read gets a 64-bit list of the members still to score;
//   4  second round: per member with a non-empty list, a compact batch of its listed reads in read-id order, the score pass, and
//      panel_merge_kernel, which replaces the held result iff the new one ranks strictly higher, or ranks equal and comes from a
//      lower member — so the answer does not depend on the order of the merges.
// The proof only decides what a read costs: a member without a usable index has no bound, and with ZSW_OPTION_EXACT_PRUNING off no
// member has one, p = 0 and every read is scored against every member; the results are the same. Host model of the decision:
// tests/models/panel_bound.cpp.
#include <hipcub/hipcub.hpp>

#include "zsw_panel.hpp"
#include "zsw_wave.hpp"

using namespace zsw;
using namespace zsw::capi;

namespace {

static_assert(PANEL_MAX_REFS == ZSW_PANEL_MAX_REFS, "one bit per member in a read's list");
constexpr uint32_t PANEL_STAGE_LEN = 160;  // as seed_kernel: contiguous fixed-length reads of up to this many bases arrive through LDS

struct PanelSeedArgs {
    const uint8_t* bases;
    const uint64_t* offsets;  // null: fixed_len
    uint32_t fixed_len;
    uint32_t n;
    const ScoringDev* sc;
    const PanelMemberDev* members;
    uint32_t n_refs;
    uint32_t min_len;
    uint8_t* first;    // [read]
    uint16_t* bounds;  // [read * n_refs + member]: seed_bound_u16
    int32_t* dbg;
};

// One thread per read, the block's reads staged through LDS as in strand_seed_kernel<true>. The members take turns: the block
// builds the member's byte -> cell table, every thread sweeps its read under the member's parameters (members with the parameters
// of the one before reuse the sweep) and has the member's sixteen index entries in flight together.
template <bool STAGED>
__global__ __launch_bounds__(256) void panel_seed_kernel(PanelSeedArgs a) {
    __shared__ uint16_t lut[256];  // byte -> potential | code << 8 (0xff: not a good residue) under the current member
    __shared__ __attribute__((aligned(16))) uint8_t sbytes[STAGED ? 256 * PANEL_STAGE_LEN + 16 : 16];
    const PanelMemberDev* __restrict__ members = a.members;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < a.n;
    uint32_t len = 0;
    uint64_t off = 0;
    if (valid) {
        off = a.offsets ? a.offsets[i] : (uint64_t)i * a.fixed_len;
        len = a.offsets ? (uint32_t)(a.offsets[i + 1] - off) : a.fixed_len;
    }
    if (STAGED) {  // bytes [block_first * L, min(n, block_first + 256) * L) of the batch, 16 at a time, head and tail byte by byte
        const uint32_t L = a.fixed_len;
        const uint64_t b0 = (uint64_t)(blockIdx.x * 256u) * L;
        const uint32_t cnt = min(256u, a.n - blockIdx.x * 256u) * L;
        const uint8_t* src = a.bases + b0;
        const uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u);
        const uint32_t shift = (16u - head) & 15u;  // LDS offset = global offset + shift: aligned loads land on aligned stores
        for (uint32_t k = threadIdx.x; k < min(head, cnt); k += 256) sbytes[shift + k] = src[k];
        const uint32_t n16 = cnt > head ? (cnt - head) / 16 : 0;
        for (uint32_t k = threadIdx.x; k < n16; k += 256)
            *reinterpret_cast<uint4*>(&sbytes[shift + head + 16 * k]) = *reinterpret_cast<const uint4*>(src + head + 16 * k);
        for (uint32_t k = head + 16 * n16 + threadIdx.x; k < cnt; k += 256) sbytes[shift + k] = src[k];
        off = (uint64_t)shift + (uint64_t)threadIdx.x * L;
    }
    const uint8_t* bases = STAGED ? sbytes + off : a.bases + off;
    const int n = (int)len;
    const uint32_t K = a.n_refs;
    const uint8_t residue = a.sc->index_map[threadIdx.x];
    SeedSweep s;
    s.m = 0;
    int best = 0;
    uint32_t p = 0;
    int32_t* rec = a.dbg && valid ? a.dbg + (2 + 2 * (size_t)K) * i : nullptr;
    for (uint32_t k = 0; k < K; ++k) {  // k, and with it every branch on the member's own fields, is uniform across the block
        const PanelMemberDev* m = members + k;
        const uint2* table = m->table;
        uint32_t u16 = 0xffffu;
        int support = 0;
        if (table) {
            if (!m->same_sweep) {
                __syncthreads();  // the staged bytes are in place; nobody still sweeps under the table of the member before
                lut[threadIdx.x] = (uint16_t)seed_cell(m->sp, (int)residue);
                __syncthreads();
                if (valid) seed_whole_sweep(m->sp, n, (int)a.min_len, [&](int c) { return (uint32_t)lut[bases[c]]; }, &s);
            }
            if (valid) {
                uint32_t f1[SEED_MAX_KMERS], l1[SEED_MAX_KMERS];
#pragma unroll
                for (int j = 0; j < SEED_MAX_KMERS; ++j) {
                    const uint2 e = table[s.codes[j]];
                    f1[j] = e.x;
                    l1[j] = e.y;
                }
                const SeedWhole w = seed_whole_finish(m->sp, s, f1, l1);
                u16 = seed_bound_u16(w.u);
                support = w.support;
            }
        }
        if (valid) {
            a.bounds[(size_t)i * K + k] = (uint16_t)u16;
            if (support > best) {  // ties stay with the lowest member
                best = support;
                p = k;
            }
            if (rec) {
                rec[2 + k] = support;
                rec[2 + K + k] = u16 == 0xffffu ? -1 : (int32_t)u16;
            }
        }
    }
    if (valid) {
        a.first[i] = (uint8_t)p;
        if (rec) {
            rec[0] = (int32_t)p;
            rec[1] = 0;
        }
    }
}

// no member has a usable index (or exact pruning is off): every read goes to member 0 first and has no bound
__global__ void panel_nobound_kernel(uint32_t n, uint32_t n_refs, uint8_t* first, uint16_t* bounds, int32_t* dbg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    first[i] = 0;
    for (uint32_t k = 0; k < n_refs; ++k) bounds[(size_t)i * n_refs + k] = 0xffffu;
    if (dbg) {
        int32_t* r = dbg + (2 + 2 * (size_t)n_refs) * i;
        r[0] = r[1] = 0;
        for (uint32_t k = 0; k < n_refs; ++k) {
            r[2 + k] = 0;
            r[2 + n_refs + k] = -1;
        }
    }
}

// the sizes of the first round's groups: a histogram of `first` per block in LDS, one atomic per block and member with reads
__global__ __launch_bounds__(256) void panel_group_sizes_kernel(uint32_t n, const uint8_t* first, uint32_t* counts) {
    __shared__ uint32_t h[PANEL_MAX_REFS];
    if (threadIdx.x < PANEL_MAX_REFS) h[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) atomicAdd(&h[first[i] & (PANEL_MAX_REFS - 1)], 1u);
    __syncthreads();
    if (threadIdx.x < PANEL_MAX_REFS && h[threadIdx.x]) atomicAdd(counts + PC_ROUND1 + threadIdx.x, h[threadIdx.x]);
}

struct PanelSettleArgs {
    uint32_t n, n_refs;
    const uint8_t* first;
    const uint16_t* bounds;
    const uint32_t* score;
    const uint8_t* status;
    unsigned long long* todo;
    uint32_t* counts;
    int use_bounds;
    int32_t* dbg;
};

// A wavefront walks groups of 64 reads (grid stride) and keeps its counts in registers — lane k the length of member k's list, the
// two others in every lane —: one atomic per wavefront and counter, at the end. (One per group of 64 reads, all on the same few
// addresses, took 9.6 ms for 10 M reads and 8 members.)
__global__ __launch_bounds__(256) void panel_settle_kernel(PanelSettleArgs a) {
    const uint32_t K = a.n_refs;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t listed = 0, settled = 0, all = 0;
    for (uint32_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; base < a.n; base += gridDim.x * 256u) {
        const uint32_t i = base + lane;
        const bool valid = i < a.n;
        unsigned long long todo = 0;
        if (valid) {
            const int p = a.first[i];
            if (a.use_bounds) todo = seed_panel_todo((int)K, p, a.status[i] == ZSW_STATUS_SOME, (long long)a.score[i], a.bounds + (size_t)i * K);
            else todo = (K >= 64 ? ~0ull : (1ull << K) - 1ull) & ~(1ull << p);
            a.todo[i] = todo;
            if (a.dbg) a.dbg[(2 + 2 * (size_t)K) * i + 1] = todo == 0 ? 1 : 0;
        }
        settled += (uint32_t)__popcll(__ballot(valid && todo == 0));
        all += (uint32_t)__popcll(__ballot(valid && (uint32_t)__popcll(todo) == K - 1));
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t c = (uint32_t)__popcll(__ballot((todo >> k) & 1ull));
            if (lane == k) listed += c;
        }
    }
    if (lane == 0 && settled) atomicAdd(a.counts + PC_SETTLED, settled);
    if (lane == 0 && all) atomicAdd(a.counts + PC_ALL, all);
    if (lane < K && listed) atomicAdd(a.counts + PC_ROUND2 + lane, listed);
}

// which reads a compact batch holds: those whose first choice is k, whose list holds k, or whose entry of a caller's array is k
struct PanelPick {
    const uint8_t* first;
    const unsigned long long* todo;
    const uint32_t* ref_of;
    uint32_t k;
    __host__ __device__ __forceinline__ bool operator()(const uint32_t& i) const {
        return first ? first[i] == k : todo ? ((todo[i] >> k) & 1ull) != 0 : ref_of[i] == k;
    }
};

// lengths of the listed reads, and a closing zero: their exclusive sum is the offsets of the compact batch
__global__ void panel_lengths_kernel(const uint64_t* offsets, const uint32_t* list, uint32_t n2, uint64_t* lens) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n2) return;
    lens[k] = k < n2 ? offsets[list[k] + 1] - offsets[list[k]] : 0;
}

struct PanelGatherArgs {
    const uint8_t* src;
    const uint64_t* src_off;  // null: fixed_len
    uint32_t fixed_len;
    const uint32_t* list;
    uint32_t n_items;
    uint8_t* dst;
    const uint64_t* dst_off;  // [item]; null: item * fixed_len
};

// the listed reads as a compact batch: one wavefront per read
__global__ __launch_bounds__(256) void panel_gather_kernel(PanelGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t sub = threadIdx.x >> 6;
    for (uint64_t j = (uint64_t)blockIdx.x * 4 + sub; j < a.n_items; j += (uint64_t)gridDim.x * 4) {
        const uint32_t id = wave::uni(a.list[j]);
        const uint64_t so = a.src_off ? a.src_off[id] : (uint64_t)id * a.fixed_len;
        const uint64_t len = a.src_off ? a.src_off[id + 1] - so : a.fixed_len;
        const uint64_t dof = a.dst_off ? a.dst_off[j] : j * a.fixed_len;
        wave::wave_copy(a.dst + dof, a.src + so, len, lane);
    }
}

__device__ __forceinline__ unsigned long long panel_rank(uint8_t status, uint32_t score) {
    return status == ZSW_STATUS_OVERFLOWED ? 2ull << 32 : status == ZSW_STATUS_SOME ? (1ull << 32) | score : 0ull;
}

struct PanelMergeArgs {
    uint32_t n2;
    const uint32_t* list;  // null: item j is read j
    const uint32_t* score2;
    const uint8_t* status2;
    const uint8_t* tier2;
    uint32_t* score;
    uint8_t* status;
    uint8_t* tier;  // may be null
    uint32_t* ref;
    uint32_t k;
    int first_round;  // the reads hold no result yet
};

// the results of member k for the listed reads: taken iff they rank strictly higher than what the read holds, or equal from a lower member
__global__ __launch_bounds__(256) void panel_merge_kernel(PanelMergeArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n2) return;
    const uint32_t id = a.list ? a.list[j] : j;
    bool take = a.first_round != 0;
    if (!take) {
        const unsigned long long held = panel_rank(a.status[id], a.score[id]), mine = panel_rank(a.status2[j], a.score2[j]);
        take = mine > held || (mine == held && a.k < a.ref[id]);
    }
    if (take) {
        a.score[id] = a.score2[j];
        a.status[id] = a.status2[j];
        if (a.tier) a.tier[id] = a.tier2[j];
        a.ref[id] = a.k;
    }
}

Panel* panel_of(zsw_context* ctx) {
    if (!ctx->panel) ctx->panel = new (std::nothrow) Panel();
    return ctx->panel;
}

Against against_member(zsw_context* ctx, Panel* P, uint32_t k) {
    PanelMember& m = P->members[k];
    return Against{P->d_seqs.as<uint8_t>() + m.start, P->h_seqs.data() + m.start, (size_t)m.len, ctx->d_sc.as<ScoringDev>(), &ctx->h_sc, &m.index, true, true};
}

// arguments every panel call checks before it touches the device
zsw_error check_panel_batch(zsw_context* ctx, const zsw_batch* reads) {
    if (!reads) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (reads->encoding == ZSW_ENCODING_PACKED4) return fail(ctx, ZSW_ERR_UNSUPPORTED, "panel calls take ZSW_ENCODING_BYTES");
    if (reads->encoding != ZSW_ENCODING_BYTES) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.encoding");
    if (reads->n_reads > 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_reads > 2^31-1 per call");
    if (reads->n_reads && !reads->bases) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null bases");
    if (reads->mem == ZSW_MEM_HOST && reads->offsets && !offsets_monotone(reads->offsets, reads->n_reads)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
    return ZSW_OK;
}

// the ascending ids of the reads `pick` names, to PW_LIST (or `list`); their number to PW_NSEL
zsw_error select_reads(zsw_context* ctx, Panel* P, uint32_t n, const PanelPick& pick, uint32_t* list, hipStream_t stream) {
    DevBuf* ws = P->ws;
    ZSW_HIP(ctx, ws[PW_NSEL].ensure(16));
    hipcub::CountingInputIterator<uint32_t> ids(0u);
    size_t temp_bytes = 0;
    ZSW_HIP(ctx, hipcub::DeviceSelect::If(nullptr, temp_bytes, ids, list, ws[PW_NSEL].as<uint32_t>(), (int)n, pick, stream));
    ZSW_HIP(ctx, ws[PW_SEL_TMP].ensure(temp_bytes + 16));
    ZSW_HIP(ctx, hipcub::DeviceSelect::If(ws[PW_SEL_TMP].p, temp_bytes, ids, list, ws[PW_NSEL].as<uint32_t>(), (int)n, pick, stream));
    return ZSW_OK;
}

// the n_g listed reads of a device batch as a compact batch at `dst` (fixed length stays fixed; a ragged batch gets the offsets
// `dst_off`, n_g + 1 of them, from an exclusive sum of the lengths)
zsw_error gather_reads(zsw_context* ctx, Panel* P, const zsw_batch* reads, const uint32_t* list, uint32_t n_g, uint8_t* dst, uint64_t* dst_off, hipStream_t stream) {
    DevBuf* ws = P->ws;
    PanelGatherArgs g{};
    g.src = reads->bases;
    g.src_off = reads->offsets;
    g.fixed_len = reads->fixed_len;
    g.list = list;
    g.n_items = n_g;
    g.dst = dst;
    if (reads->offsets) {
        ZSW_HIP(ctx, ws[PW_GROUP_OFF].ensure(2 * ((size_t)n_g + 1) * 8));
        uint64_t* lens = ws[PW_GROUP_OFF].as<uint64_t>();
        hipLaunchKernelGGL(panel_lengths_kernel, dim3((n_g + 256) / 256), dim3(256), 0, stream, reads->offsets, list, n_g, lens);
        ZSW_HIP(ctx, hipGetLastError());
        size_t temp_bytes = 0;
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, lens, dst_off, (int)(n_g + 1), stream));
        ZSW_HIP(ctx, ws[PW_SCAN_TMP].ensure(temp_bytes + 16));
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[PW_SCAN_TMP].p, temp_bytes, lens, dst_off, (int)(n_g + 1), stream));
        g.dst_off = dst_off;
    }
    if (n_g) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_g + 3) / 4, 1u << 20);
        hipLaunchKernelGGL(panel_gather_kernel, dim3(grid), dim3(256), 0, stream, g);
        ZSW_HIP(ctx, hipGetLastError());
    }
    return ZSW_OK;
}

struct PanelOut {
    uint32_t* score;
    uint8_t *status, *tier;  // tier: may be null
    uint32_t* ref;
};

// One member's share of a round: the n_g reads `pick` names (every read if n_g == n) against member k, merged into `out`
zsw_error score_member(zsw_context* ctx, Panel* P, const zsw_batch* reads, size_t total, uint32_t k, const PanelPick& pick, uint32_t n_g, bool first_round,
                       const ResultRule& rule, const PanelOut& out, hipStream_t stream) {
    DevBuf* ws = P->ws;
    const uint32_t n = (uint32_t)reads->n_reads;
    ZSW_HIP(ctx, ws[PW_G_SCORE].ensure((size_t)n_g * 4 + 4));
    ZSW_HIP(ctx, ws[PW_G_STATUS].ensure((size_t)n_g + 4));
    if (out.tier) ZSW_HIP(ctx, ws[PW_G_TIER].ensure((size_t)n_g + 4));
    zsw_batch group = *reads;
    const uint32_t* list = nullptr;
    if (n_g < n) {
        ZSW_HIP(ctx, ws[PW_LIST].ensure((size_t)n * 4 + 4));
        ZSW_HIP(ctx, ws[PW_GROUP].ensure(total + 16));
        uint32_t* l = ws[PW_LIST].as<uint32_t>();
        if (zsw_error ze = select_reads(ctx, P, n, pick, l, stream); ze != ZSW_OK) return ze;
        uint64_t* offs = nullptr;
        if (reads->offsets) {
            ZSW_HIP(ctx, ws[PW_GROUP_OFF].ensure(2 * ((size_t)n_g + 1) * 8));
            offs = ws[PW_GROUP_OFF].as<uint64_t>() + n_g + 1;
        }
        if (zsw_error ze = gather_reads(ctx, P, reads, l, n_g, ws[PW_GROUP].as<uint8_t>(), offs, stream); ze != ZSW_OK) return ze;
        group.bases = ws[PW_GROUP].as<uint8_t>();
        group.offsets = offs;
        group.n_reads = n_g;
        list = l;
    }
    const ScoreDest dest{ws[PW_G_SCORE].as<uint32_t>(), ws[PW_G_STATUS].as<uint8_t>(), out.tier ? ws[PW_G_TIER].as<uint8_t>() : nullptr, nullptr, nullptr};
    if (zsw_error ze = run_score(ctx, against_member(ctx, P, k), &group, rule, dest, stream); ze != ZSW_OK) return ze;
    PanelMergeArgs m;
    m.n2 = n_g;
    m.list = list;
    m.score2 = dest.score;
    m.status2 = dest.status;
    m.tier2 = dest.tier;
    m.score = out.score;
    m.status = out.status;
    m.tier = out.tier;
    m.ref = out.ref;
    m.k = k;
    m.first_round = first_round ? 1 : 0;
    hipLaunchKernelGGL(panel_merge_kernel, dim3((n_g + 255) / 256), dim3(256), 0, stream, m);
    ZSW_HIP(ctx, hipGetLastError());
    return ZSW_OK;
}

// The panel score pass over a batch in device memory; `total`: bytes of its bases. Results to device arrays (tier may be null).
zsw_error score_panel_device(zsw_context* ctx, Panel* P, const zsw_batch* reads, size_t total, const ResultRule& rule, const PanelOut& out, hipStream_t stream) {
    const uint32_t n = (uint32_t)reads->n_reads, L = reads->fixed_len, K = (uint32_t)P->members.size();
    DevBuf* ws = P->ws;
    for (uint64_t& c : P->counts) c = 0;
    if (n == 0) return ZSW_OK;
    ZSW_HIP(ctx, ws[PW_COUNTS].ensure(PC_N * 4));
    ZSW_HIP(ctx, hipMemsetAsync(ws[PW_COUNTS].p, 0, PC_N * 4, stream));
    ZSW_HIP(ctx, ws[PW_FIRST].ensure((size_t)n + 4));
    ZSW_HIP(ctx, ws[PW_BOUNDS].ensure((size_t)n * K * 2 + 4));
    ZSW_HIP(ctx, ws[PW_TODO].ensure((size_t)n * 8 + 8));
    uint32_t* counts = ws[PW_COUNTS].as<uint32_t>();
    uint8_t* first = ws[PW_FIRST].as<uint8_t>();
    uint16_t* bounds = ws[PW_BOUNDS].as<uint16_t>();
    const uint32_t g256 = (n + 255) / 256;
    // the bounds need the members' indices (built here if no call has needed them yet)
    bool use_bounds = (ctx->flags() & ZSW_DEBUG_SCORE_PRUNE) != 0;
    if (use_bounds) {
        std::vector<PanelMemberDev>& md = P->h_members;  // (outlives the copy below)
        md.resize(K);
        bool any = false;
        for (uint32_t k = 0; k < K; ++k) {
            PanelMember& m = P->members[k];
            if (!m.index.valid) ZSW_HIP(ctx, seed_index_update(&m.index, ctx->h_sc, P->h_seqs.data() + m.start, (size_t)m.len));
            memset(&md[k], 0, sizeof(PanelMemberDev));
            md[k].sp = m.index.params;
            md[k].table = m.index.usable ? reinterpret_cast<const uint2*>(m.index.d_table) : nullptr;
            md[k].same_sweep = k > 0 && md[k].table && md[k - 1].table && memcmp(&md[k].sp, &md[k - 1].sp, sizeof(SeedParams)) == 0 ? 1u : 0u;
            any = any || md[k].table;
        }
        use_bounds = any;
        if (use_bounds) {
            ZSW_HIP(ctx, ws[PW_MEMBERS].ensure(PANEL_MAX_REFS * sizeof(PanelMemberDev)));
            ZSW_HIP(ctx, hipMemcpyAsync(ws[PW_MEMBERS].p, md.data(), K * sizeof(PanelMemberDev), hipMemcpyHostToDevice, stream));
            PanelSeedArgs s;
            s.bases = reads->bases;
            s.offsets = reads->offsets;
            s.fixed_len = L;
            s.n = n;
            s.sc = ctx->d_sc.as<ScoringDev>();
            s.members = ws[PW_MEMBERS].as<PanelMemberDev>();
            s.n_refs = K;
            s.min_len = SEED_MIN_LEN;
            s.first = first;
            s.bounds = bounds;
            s.dbg = ctx->panel_dbg;
            if (!reads->offsets && L <= PANEL_STAGE_LEN) hipLaunchKernelGGL(panel_seed_kernel<true>, dim3(g256), dim3(256), 0, stream, s);
            else hipLaunchKernelGGL(panel_seed_kernel<false>, dim3(g256), dim3(256), 0, stream, s);
            ZSW_HIP(ctx, hipGetLastError());
        }
    }
    if (!use_bounds) {
        hipLaunchKernelGGL(panel_nobound_kernel, dim3(g256), dim3(256), 0, stream, n, K, first, bounds, ctx->panel_dbg);
        ZSW_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(panel_group_sizes_kernel, dim3(std::min<uint32_t>(g256, 1024)), dim3(256), 0, stream, n, first, counts);
    ZSW_HIP(ctx, hipGetLastError());
    uint32_t h_counts[PC_N];
    // the first synchronisation of the call: the sizes of the groups
    ZSW_HIP(ctx, hipMemcpyAsync(h_counts, counts, PC_N * 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    uint64_t sum = 0;
    for (uint32_t k = 0; k < K; ++k) sum += h_counts[PC_ROUND1 + k];
    if (sum != n) return fail(ctx, ZSW_ERR_HIP, "panel pass: the first round's groups do not add up to the batch");
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t n_g = h_counts[PC_ROUND1 + k];
        if (!n_g) continue;
        const PanelPick pick{first, nullptr, nullptr, k};
        if (zsw_error ze = score_member(ctx, P, reads, total, k, pick, n_g, true, rule, out, stream); ze != ZSW_OK) return ze;
    }
    P->counts[1] = n;
    PanelSettleArgs se;
    se.n = n;
    se.n_refs = K;
    se.first = first;
    se.bounds = bounds;
    se.score = out.score;
    se.status = out.status;
    se.todo = ws[PW_TODO].as<unsigned long long>();
    se.counts = counts;
    se.use_bounds = use_bounds ? 1 : 0;
    se.dbg = ctx->panel_dbg;
    hipLaunchKernelGGL(panel_settle_kernel, dim3(std::min<uint32_t>(g256, 4096)), dim3(256), 0, stream, se);
    ZSW_HIP(ctx, hipGetLastError());
    // the second synchronisation: the lengths of the members' lists
    ZSW_HIP(ctx, hipMemcpyAsync(h_counts, counts, PC_N * 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    P->counts[0] = h_counts[PC_SETTLED];
    P->counts[3] = h_counts[PC_ALL];
    for (uint32_t k = 0; k < K; ++k) {
        const uint32_t n_g = h_counts[PC_ROUND2 + k];
        if (!n_g) continue;
        if (n_g > n) return fail(ctx, ZSW_ERR_HIP, "panel pass: a member's list is longer than the batch");
        P->counts[2] += n_g;
        const PanelPick pick{nullptr, se.todo, nullptr, k};
        if (zsw_error ze = score_member(ctx, P, reads, total, k, pick, n_g, false, rule, out, stream); ze != ZSW_OK) return ze;
    }
    return ZSW_OK;
}

// bytes of a batch's bases (a ragged device batch: its last offset comes back from the device)
zsw_error panel_batch_bytes(zsw_context* ctx, const zsw_batch* reads, hipStream_t stream, size_t* total) {
    const uint64_t n = reads->n_reads;
    if (!reads->offsets) {
        *total = (size_t)n * reads->fixed_len;
    } else if (reads->mem == ZSW_MEM_HOST) {
        *total = (size_t)reads->offsets[n];
    } else {
        uint64_t last = 0;
        ZSW_HIP(ctx, hipMemcpyAsync(&last, reads->offsets + n, 8, hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
        *total = (size_t)last;
    }
    return ZSW_OK;
}

// zsw_score_panel_batch_from for host and device batches
zsw_error score_panel(zsw_context* ctx, Panel* P, const zsw_batch* reads, const ResultRule& rule, uint32_t* out_score, uint8_t* out_status, uint8_t* out_tier,
                      uint32_t* out_ref, hipStream_t stream) {
    if (!reads->offsets && reads->fixed_len == 0 && reads->n_reads) return fail(ctx, ZSW_ERR_EMPTY_SEQUENCE, "fixed-length batch of empty reads");
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    size_t total = 0;
    zsw_error ze = panel_batch_bytes(ctx, reads, stream, &total);
    if (ze != ZSW_OK) return ze;
    if (reads->mem != ZSW_MEM_HOST) return score_panel_device(ctx, P, reads, total, rule, {out_score, out_status, out_tier, out_ref}, stream);
    // a host batch: the bases cross once, both rounds and the kernels between them run on the device copy
    const size_t n = reads->n_reads;
    DevBuf* ws = P->ws;
    ZSW_HIP(ctx, ws[PW_IN].ensure(total + 16));
    ZSW_HIP(ctx, ws[PW_OUT_SCORE].ensure(n * 4 + 4));
    ZSW_HIP(ctx, ws[PW_OUT_STATUS].ensure(n + 4));
    ZSW_HIP(ctx, ws[PW_OUT_TIER].ensure(n + 4));
    ZSW_HIP(ctx, ws[PW_OUT_REF].ensure(n * 4 + 4));
    if (total) ZSW_HIP(ctx, hipMemcpyAsync(ws[PW_IN].p, reads->bases, total, hipMemcpyHostToDevice, stream));
    zsw_batch dev = *reads;
    dev.mem = ZSW_MEM_DEVICE;
    dev.bases = ws[PW_IN].as<uint8_t>();
    if (reads->offsets) {
        ZSW_HIP(ctx, ws[PW_IN_OFF].ensure((n + 1) * 8));
        ZSW_HIP(ctx, hipMemcpyAsync(ws[PW_IN_OFF].p, reads->offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
        dev.offsets = ws[PW_IN_OFF].as<uint64_t>();
    }
    ze = score_panel_device(ctx, P, &dev, total, rule,
                            {ws[PW_OUT_SCORE].as<uint32_t>(), ws[PW_OUT_STATUS].as<uint8_t>(), out_tier ? ws[PW_OUT_TIER].as<uint8_t>() : nullptr, ws[PW_OUT_REF].as<uint32_t>()},
                            stream);
    if (ze != ZSW_OK || n == 0) return ze;
    ZSW_HIP(ctx, hipMemcpyAsync(out_score, ws[PW_OUT_SCORE].p, n * 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipMemcpyAsync(out_status, ws[PW_OUT_STATUS].p, n, hipMemcpyDeviceToHost, stream));
    if (out_tier) ZSW_HIP(ctx, hipMemcpyAsync(out_tier, ws[PW_OUT_TIER].p, n, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipMemcpyAsync(out_ref, ws[PW_OUT_REF].p, n * 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    return ZSW_OK;
}

}  // namespace

namespace zsw {
namespace capi {

void panel_invalidate(zsw_context* ctx) {
    if (!ctx || !ctx->panel) return;
    for (PanelMember& m : ctx->panel->members) m.index.valid = false;
}

void panel_release(zsw_context* ctx) {
    if (!ctx || !ctx->panel) return;
    for (PanelMember& m : ctx->panel->members) seed_index_release(&m.index);
    ctx->panel->d_seqs.release();
    for (DevBuf& b : ctx->panel->ws) b.release();
    delete ctx->panel;
    ctx->panel = nullptr;
}

}  // namespace capi
}  // namespace zsw

extern "C" {

zsw_error zsw_set_panel(zsw_context* ctx, const uint8_t* seqs, const uint64_t* offsets, uint32_t n_refs, zsw_mem mem) {
    DeviceGuard device_guard(ctx);
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (!seqs || !offsets) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (n_refs == 0 || n_refs > PANEL_MAX_REFS) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_refs must be 1 .. ZSW_PANEL_MAX_REFS");
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)n_refs + 1);
    if (mem == ZSW_MEM_HOST) memcpy(off.data(), offsets, off.size() * 8);
    else ZSW_HIP(ctx, hipMemcpy(off.data(), offsets, off.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < n_refs; ++k) {
        if (off[k + 1] < off[k]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
        if (off[k + 1] - off[k] > 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "panel member too long");
    }
    for (uint32_t k = 0; k < n_refs; ++k)
        if (off[k + 1] == off[k]) return fail(ctx, ZSW_ERR_EMPTY_SEQUENCE, "empty panel member");
    Panel* P = panel_of(ctx);
    if (!P) return fail(ctx, ZSW_ERR_HIP, "out of host memory");
    if (!P->members.empty()) ZSW_HIP(ctx, hipDeviceSynchronize());  // queued kernels may still read the previous panel
    for (PanelMember& m : P->members) seed_index_release(&m.index);
    P->members.clear();
    std::vector<PanelMember> members(n_refs);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_refs; ++k) {
        members[k].start = at;
        members[k].len = off[k + 1] - off[k];
        at = (at + members[k].len + 16 + 255) / 256 * 256;
    }
    ZSW_HIP(ctx, P->d_seqs.ensure((size_t)at + 16));
    P->h_seqs.assign((size_t)at + 16, 0);
    for (uint32_t k = 0; k < n_refs; ++k) {
        const PanelMember& m = members[k];
        uint8_t* d = P->d_seqs.as<uint8_t>() + m.start;
        if (mem == ZSW_MEM_HOST) {
            memcpy(P->h_seqs.data() + m.start, seqs + off[k], (size_t)m.len);
            ZSW_HIP(ctx, hipMemcpy(d, seqs + off[k], (size_t)m.len, hipMemcpyHostToDevice));
        } else {  // a device array is taken where it lies
            ZSW_HIP(ctx, hipMemcpy(d, seqs + off[k], (size_t)m.len, hipMemcpyDeviceToDevice));
            ZSW_HIP(ctx, hipMemcpy(P->h_seqs.data() + m.start, seqs + off[k], (size_t)m.len, hipMemcpyDeviceToHost));
        }
    }
    P->members.swap(members);
    for (uint64_t& c : P->counts) c = 0;
    return ZSW_OK;
}

zsw_error zsw_score_panel_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, uint32_t* out_score, uint8_t* out_status,
                                     uint8_t* out_tier, uint32_t* out_ref, void* stream) {
    DeviceGuard device_guard(ctx);
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (zsw_error ze = min_score_unsupported(ctx, "zsw_score_panel_batch_from"); ze != ZSW_OK) return ze;
    if (!ctx->scoring_set || !ctx->panel || ctx->panel->members.empty()) return fail(ctx, ZSW_ERR_NOT_CONFIGURED, "scoring/panel not set");
    if (zsw_error ze = check_panel_batch(ctx, reads); ze != ZSW_OK) return ze;
    if (!out_score || !out_status || !out_ref) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    ResultRule rule;
    if (zsw_error ze = rule_cascade(ctx, from_width, preset_bits, &rule); ze != ZSW_OK) return ze;
    return score_panel(ctx, ctx->panel, reads, rule, out_score, out_status, out_tier, out_ref, (hipStream_t)stream);
}

zsw_error zsw_panel_gather_batch(zsw_context* ctx, const zsw_batch* reads, const uint32_t* ref_of, uint32_t k, uint8_t* out_bases, uint64_t* out_offsets,
                                 uint32_t* out_index, uint64_t* out_n, void* stream_) {
    DeviceGuard device_guard(ctx);
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (zsw_error ze = check_panel_batch(ctx, reads); ze != ZSW_OK) return ze;
    if (!out_n) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    *out_n = 0;
    const uint64_t n = reads->n_reads;
    if (n == 0) {
        if (reads->offsets && out_offsets && reads->mem == ZSW_MEM_HOST) out_offsets[0] = 0;
        return ZSW_OK;
    }
    if (!ref_of || !out_bases || !out_index || (reads->offsets && !out_offsets)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (reads->mem == ZSW_MEM_HOST) {
        uint64_t m = 0, at = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (ref_of[i] != k) continue;
            const uint64_t off = reads->offsets ? reads->offsets[i] : i * reads->fixed_len;
            const uint64_t len = reads->offsets ? reads->offsets[i + 1] - off : reads->fixed_len;
            memcpy(out_bases + at, reads->bases + off, len);
            if (reads->offsets) out_offsets[m] = at;
            out_index[m++] = (uint32_t)i;
            at += len;
        }
        if (reads->offsets) out_offsets[m] = at;
        *out_n = m;
        return ZSW_OK;
    }
    hipStream_t stream = (hipStream_t)stream_;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    Panel* P = panel_of(ctx);
    if (!P) return fail(ctx, ZSW_ERR_HIP, "out of host memory");
    const PanelPick pick{nullptr, nullptr, ref_of, k};
    if (zsw_error ze = select_reads(ctx, P, (uint32_t)n, pick, out_index, stream); ze != ZSW_OK) return ze;
    uint32_t m = 0;  // the one synchronisation of the call: how many reads the group holds
    ZSW_HIP(ctx, hipMemcpyAsync(&m, P->ws[PW_NSEL].p, 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    if (m > n) return fail(ctx, ZSW_ERR_HIP, "panel gather: more reads selected than the batch holds");
    *out_n = m;
    return gather_reads(ctx, P, reads, out_index, m, out_bases, reads->offsets ? out_offsets : nullptr, stream);
}

zsw_error zsw_panel_counts(zsw_context* ctx, uint64_t* out) {
    if (!ctx || !out) return ZSW_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 4; ++k) out[k] = ctx->panel ? ctx->panel->counts[k] : 0;
    return ZSW_OK;
}

zsw_error zsw_debug_panel_records(zsw_context* ctx, int32_t* records) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    ctx->panel_dbg = records;
    return ZSW_OK;
}

}  // extern "C"
