// zsw_strand.hip — reads from either strand (include/zoe_sw.h: zsw_score_strands_batch_from, zsw_orient_batch,
// zsw_align_3pass_strands_batch_from). The contract: F = f(read), R = f(rc(read)) for an existing entry point f; the answer is F
// unless R ranks strictly higher (OVERFLOWED > SOME by score > UNMAPPED = EMPTY), bit for bit what f returns for that orientation.
//
// Scoring both orientations of every read doubles the work. Instead, per read:
//   1  strand_seed_kernel sweeps the read and its reverse complement as seed_kernel sweeps a read (zsw_seed.hpp: seed_whole_sweep),
//      looks the sampled k-mers of both up in the reference index and keeps, per orientation, the support of the anchor vote and
//      claim W's bound U: no local alignment of that orientation against the reference scores more than U;
//   2  the orientation with more support (ties: forward) is written by strand_orient_kernel and scored by the existing score pass;
//   3  strand_settle_kernel: if that score is SOME and beyond the other orientation's U (or equal to it, when the tie rule favours
//      the first orientation anyway), the other orientation cannot win and is never computed; every other read is listed;
//   4  the listed reads' other orientation is written into a second, compacted batch, scored by the existing score pass, and
//      strand_merge_kernel applies the ranking.
// The proof only decides what a read costs: with no usable index, or with ZSW_OPTION_EXACT_PRUNING off, every read is listed and
// the results are the same. Host model of claim W and of the decision: tests/models/strand_bound.cpp.
#include <hipcub/hipcub.hpp>

#include "zsw_context.hpp"
#include "zsw_strand.hpp"

using namespace zsw;
using namespace zsw::capi;

namespace {

constexpr uint32_t STRAND_STAGE_LEN = 160;  // as seed_kernel: contiguous fixed-length reads of up to this many bases arrive through LDS

struct StrandSeedArgs {
    BatchDev b;
    const ScoringDev* sc;
    SeedParams sp;
    const uint2* table;
    uint32_t n;
    uint32_t min_len;
    uint2* meta;
    int32_t* dbg;
    ComplementTable ct;
};

// One thread per read, the block's reads staged through LDS as in seed_kernel<true>. Column c of the reverse complement is the
// complement of base len - 1 - c: the complement is applied to the byte in front of the cell look-up, i.e. the second table is
// lut[complement[byte]], built once per block.
template <bool STAGED>
__global__ __launch_bounds__(256) void strand_seed_kernel(StrandSeedArgs a) {
    __shared__ uint16_t lut_f[256], lut_r[256];  // byte -> potential | code << 8 (0xff: not a good residue), forward / complemented
    __shared__ __attribute__((aligned(16))) uint8_t sbytes[STAGED ? 256 * STRAND_STAGE_LEN + 16 : 16];
    {
        const uint32_t cellv = seed_cell(a.sp, (int)a.sc->index_map[threadIdx.x]);
        lut_f[threadIdx.x] = (uint16_t)cellv;
        const uint32_t cellc = seed_cell(a.sp, (int)a.sc->index_map[a.ct.t[threadIdx.x]]);
        lut_r[threadIdx.x] = (uint16_t)cellc;
    }
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < a.n;
    uint32_t len = 0;
    uint64_t off = 0;
    if (valid) {
        off = a.b.offsets ? a.b.offsets[i] : (uint64_t)i * a.b.fixed_len;
        len = a.b.offsets ? (uint32_t)(a.b.offsets[i + 1] - off) : a.b.fixed_len;
    }
    if (STAGED) {  // bytes [block_first * L, min(n, block_first + 256) * L) of the batch, 16 at a time, head and tail byte by byte
        const uint32_t L = a.b.fixed_len;
        const uint64_t b0 = (uint64_t)(blockIdx.x * 256u) * L;
        const uint32_t cnt = min(256u, a.n - blockIdx.x * 256u) * L;
        const uint8_t* src = a.b.bases + b0;
        const uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u);
        const uint32_t shift = (16u - head) & 15u;  // LDS offset = global offset + shift: aligned loads land on aligned stores
        for (uint32_t k = threadIdx.x; k < min(head, cnt); k += 256) sbytes[shift + k] = src[k];
        const uint32_t n16 = cnt > head ? (cnt - head) / 16 : 0;
        for (uint32_t k = threadIdx.x; k < n16; k += 256)
            *reinterpret_cast<uint4*>(&sbytes[shift + head + 16 * k]) = *reinterpret_cast<const uint4*>(src + head + 16 * k);
        for (uint32_t k = head + 16 * n16 + threadIdx.x; k < cnt; k += 256) sbytes[shift + k] = src[k];
        off = (uint64_t)shift + (uint64_t)threadIdx.x * L;
    }
    __syncthreads();
    if (!valid) return;
    const uint8_t* bases = STAGED ? sbytes + off : a.b.bases + off;
    const int n = (int)len;
    SeedSweep sf, sr;
    seed_whole_sweep(a.sp, n, (int)a.min_len, [&](int c) { return (uint32_t)lut_f[bases[c]]; }, &sf);
    seed_whole_sweep(a.sp, n, (int)a.min_len, [&](int c) { return (uint32_t)lut_r[bases[n - 1 - c]]; }, &sr);
    // the index entries of both orientations' k-mers: thirty-two independent loads in flight together
    uint32_t f1[2 * SEED_MAX_KMERS], l1[2 * SEED_MAX_KMERS];
    const uint2* table = a.table;
#pragma unroll
    for (int j = 0; j < SEED_MAX_KMERS; ++j) {
        const uint2 ef = table[sf.codes[j]], er = table[sr.codes[j]];
        f1[j] = ef.x;
        l1[j] = ef.y;
        f1[SEED_MAX_KMERS + j] = er.x;
        l1[SEED_MAX_KMERS + j] = er.y;
    }
    const SeedWhole wf = seed_whole_finish(a.sp, sf, f1, l1);
    const SeedWhole wr = seed_whole_finish(a.sp, sr, f1 + SEED_MAX_KMERS, l1 + SEED_MAX_KMERS);
    const int first = wr.support > wf.support ? 1 : 0;  // ties go forward
    const uint32_t uf = seed_bound_u16(wf.u), ur = seed_bound_u16(wr.u);
    a.meta[i] = strand_meta_pack(uf, ur, wf.support, wr.support, first);
    if (a.dbg) {
        int32_t* r = a.dbg + (size_t)STRAND_RECORD_INTS * i;
        r[0] = wf.support;
        r[1] = wr.support;
        r[2] = uf == 0xffffu ? -1 : (int32_t)uf;
        r[3] = ur == 0xffffu ? -1 : (int32_t)ur;
        r[4] = first;
    }
}

// no usable index (or exact pruning off): every read runs forward first and has no bound
__global__ void strand_nobound_kernel(uint32_t n, uint2* meta, int32_t* dbg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    meta[i] = strand_meta_pack(0xffffu, 0xffffu, 0, 0, 0);
    if (dbg) {
        int32_t* r = dbg + (size_t)STRAND_RECORD_INTS * i;
        r[0] = r[1] = r[4] = 0;
        r[2] = r[3] = -1;
    }
}

struct OrientArgs {
    const uint8_t* src;
    const uint64_t* src_off;  // null: fixed_len
    uint32_t fixed_len;
    const uint32_t* items;    // null: item k is read k
    uint32_t n_items;
    uint8_t* dst;
    const uint64_t* dst_off;  // [item]; null: the source's own offset (items == null) or k * fixed_len
    const uint8_t* strand;    // [read]: != 0 = reverse complement; null: from meta
    const uint2* meta;        // [read]: the strand that ran first, ^ flip
    uint32_t flip;
    ComplementTable ct;
};

// The oriented copy of the items: 32 lanes per read, lane t moves bytes t, t + 32, ... — consecutive lanes load consecutive bytes
// (descending for a reverse complement) and store consecutive bytes.
__global__ __launch_bounds__(256) void strand_orient_kernel(OrientArgs a) {
    __shared__ uint8_t ct[256];
    ct[threadIdx.x] = a.ct.t[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 31u, sub = threadIdx.x >> 5;
    for (uint64_t k = (uint64_t)blockIdx.x * 8 + sub; k < a.n_items; k += (uint64_t)gridDim.x * 8) {
        const uint32_t id = a.items ? a.items[k] : (uint32_t)k;
        const uint64_t so = a.src_off ? a.src_off[id] : (uint64_t)id * a.fixed_len;
        const uint32_t len = a.src_off ? (uint32_t)(a.src_off[id + 1] - so) : a.fixed_len;
        const uint64_t dof = a.dst_off ? a.dst_off[k] : (a.items ? k * a.fixed_len : so);
        const bool rc = a.strand ? a.strand[id] != 0 : ((strand_meta_first(a.meta[id]) ^ a.flip) != 0);
        const uint8_t* s = a.src + so;
        uint8_t* d = a.dst + dof;
        if (rc)
            for (uint32_t c = lane; c < len; c += 32) d[c] = ct[s[len - 1 - c]];
        else
            for (uint32_t c = lane; c < len; c += 32) d[c] = s[c];
    }
}

struct SettleArgs {
    uint32_t n;
    const uint2* meta;
    const uint32_t* score;
    const uint8_t* status;
    uint8_t* strand;
    uint32_t* list;
    uint32_t* counts;
    int use_bounds;
    int32_t* dbg;
};

__global__ __launch_bounds__(256) void strand_settle_kernel(SettleArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < a.n;
    int first = 0;
    bool settled = false;
    if (valid) {
        const uint2 m = a.meta[i];
        first = (int)strand_meta_first(m);
        const uint32_t uo = strand_meta_bound(m, 1 - first);
        settled = a.use_bounds && seed_strand_settled(a.status[i] == ZSW_STATUS_SOME, (long long)a.score[i], uo == 0xffffu ? -1ll : (long long)uo, first);
        a.strand[i] = (uint8_t)first;
        if (a.dbg) {
            int32_t* r = a.dbg + (size_t)STRAND_RECORD_INTS * i;
            r[5] = settled ? 1 : 0;
            r[6] = r[7] = 0;
        }
    }
    // one atomic per counter and wavefront; the unsettled reads of a wavefront take consecutive places of the list
    const unsigned long long mf = __ballot(valid && settled && first == 0), mr = __ballot(valid && settled && first == 1);
    const unsigned long long mu = __ballot(valid && !settled);
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) {
        if (mf) atomicAdd(a.counts + STC_SETTLED_F, (uint32_t)__popcll(mf));
        if (mr) {
            atomicAdd(a.counts + STC_SETTLED_R, (uint32_t)__popcll(mr));
            atomicAdd(a.counts + STC_REVERSE, (uint32_t)__popcll(mr));
        }
        if (mu) base = atomicAdd(a.counts + STC_BOTH, (uint32_t)__popcll(mu));
    }
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (valid && !settled) a.list[base + (uint32_t)__popcll(mu & ((1ull << lane) - 1ull))] = i;
}

// lengths of the listed reads, and a closing zero: their exclusive sum is the offsets of the second batch
__global__ void strand_lengths_kernel(const uint64_t* offsets, const uint32_t* list, uint32_t n2, uint64_t* lens) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n2) return;
    lens[k] = k < n2 ? offsets[list[k] + 1] - offsets[list[k]] : 0;
}

__device__ __forceinline__ unsigned long long strand_rank(uint8_t status, uint32_t score) {
    return status == ZSW_STATUS_OVERFLOWED ? 2ull << 32 : status == ZSW_STATUS_SOME ? (1ull << 32) | score : 0ull;
}

struct MergeArgs {
    uint32_t n2;
    const uint32_t* list;
    const uint32_t* score2;
    const uint8_t* status2;
    const uint8_t* tier2;
    uint32_t* score;
    uint8_t* status;
    uint8_t* tier;  // may be null
    uint8_t* strand;
    uint32_t* counts;
};

// the reads scored on both strands: the forward result unless the reverse one ranks strictly higher
__global__ __launch_bounds__(256) void strand_merge_kernel(MergeArgs a) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    bool reverse = false;
    if (k < a.n2) {
        const uint32_t id = a.list[k];
        const int first = a.strand[id];
        const unsigned long long r1 = strand_rank(a.status[id], a.score[id]), r2 = strand_rank(a.status2[k], a.score2[k]);
        reverse = first == 0 ? r2 > r1 : !(r2 > r1 || r2 == r1);  // first == 1: the second batch is the forward strand, which wins ties
        if ((reverse ? 1 : 0) != first) {
            a.score[id] = a.score2[k];
            a.status[id] = a.status2[k];
            if (a.tier) a.tier[id] = a.tier2[k];
            a.strand[id] = reverse ? 1 : 0;
        }
    }
    const unsigned long long m = __ballot(reverse);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.counts + STC_REVERSE, (uint32_t)__popcll(m));
}

ComplementTable complement_of(const zsw_context* ctx) {
    ComplementTable t;
    if (ctx->complement.size() == 256) memcpy(t.t, ctx->complement.data(), 256);
    else complement_default(t.t);
    return t;
}

hipError_t launch_orient(const OrientArgs& a, hipStream_t stream) {
    if (!a.n_items) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)a.n_items + 7) / 8, 1u << 20);
    hipLaunchKernelGGL(strand_orient_kernel, dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// arguments every strand call checks before it touches the device
zsw_error check_strand_batch(zsw_context* ctx, const zsw_batch* reads, bool need_config) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (need_config && (!ctx->scoring_set || !ctx->reference_set)) return fail(ctx, ZSW_ERR_NOT_CONFIGURED, "scoring/reference not set");
    if (!reads) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (reads->encoding == ZSW_ENCODING_PACKED4)
        return fail(ctx, ZSW_ERR_UNSUPPORTED, "strand-aware calls take ZSW_ENCODING_BYTES (a packed residue index has no complement byte)");
    if (reads->encoding != ZSW_ENCODING_BYTES) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.encoding");
    if (reads->n_reads > 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_reads > 2^31-1 per call");
    if (reads->n_reads && !reads->bases) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null bases");
    if (reads->mem == ZSW_MEM_HOST && reads->offsets && !offsets_monotone(reads->offsets, reads->n_reads)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
    return ZSW_OK;
}

// The strand-aware score pass over a batch in device memory; `total`: bytes of its bases. Results to device arrays (tier may be null).
zsw_error score_strands_device(zsw_context* ctx, const zsw_batch* reads, size_t total, const ResultRule& rule, uint32_t* d_score, uint8_t* d_status,
                               uint8_t* d_tier, uint8_t* d_strand, hipStream_t stream) {
    const uint32_t n = (uint32_t)reads->n_reads, L = reads->fixed_len;
    DevBuf* ws = ctx->st_ws;
    ZSW_HIP(ctx, ws[ST_COUNTS].ensure(STC_N * 4));
    ZSW_HIP(ctx, hipMemsetAsync(ws[ST_COUNTS].p, 0, STC_N * 4, stream));
    if (n == 0) return ZSW_OK;
    ZSW_HIP(ctx, ws[ST_META].ensure((size_t)n * 8 + 8));
    ZSW_HIP(ctx, ws[ST_LIST].ensure((size_t)n * 4 + 4));
    uint32_t* counts = ws[ST_COUNTS].as<uint32_t>();
    uint2* meta = ws[ST_META].as<uint2>();
    const uint32_t g256 = (n + 255) / 256;
    // the bounds need the reference index of the seeded pass (built here if no call has needed it yet)
    bool use_bounds = (ctx->flags() & ZSW_DEBUG_SCORE_PRUNE) != 0 && ctx->ref_len > 0;
    if (use_bounds && !ctx->seed.valid) ZSW_HIP(ctx, seed_index_update(&ctx->seed, ctx->h_sc, ctx->h_ref.data(), ctx->ref_len));
    use_bounds = use_bounds && ctx->seed.usable && ctx->seed.d_table != nullptr;
    const ComplementTable ct = complement_of(ctx);
    zsw_batch first = *reads;  // the batch the first score pass runs on
    if (use_bounds) {
        StrandSeedArgs s;
        s.b.bases = reads->bases;
        s.b.offsets = reads->offsets;
        s.b.fixed_len = L;
        s.b.n_reads = s.b.n_items = n;
        s.b.items = nullptr;
        s.sc = ctx->d_sc.as<ScoringDev>();
        s.sp = ctx->seed.params;
        s.table = reinterpret_cast<const uint2*>(ctx->seed.d_table);
        s.n = n;
        s.min_len = SEED_MIN_LEN;
        s.meta = meta;
        s.dbg = ctx->strand_dbg;
        s.ct = ct;
        if (!reads->offsets && L <= STRAND_STAGE_LEN) hipLaunchKernelGGL(strand_seed_kernel<true>, dim3(g256), dim3(256), 0, stream, s);
        else hipLaunchKernelGGL(strand_seed_kernel<false>, dim3(g256), dim3(256), 0, stream, s);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, ws[ST_ORIENT].ensure(total + 16));
        OrientArgs o{};
        o.src = reads->bases;
        o.src_off = reads->offsets;
        o.fixed_len = L;
        o.n_items = n;
        o.dst = ws[ST_ORIENT].as<uint8_t>();
        o.meta = meta;
        o.ct = ct;
        ZSW_HIP(ctx, launch_orient(o, stream));
        first.bases = ws[ST_ORIENT].as<uint8_t>();
    } else {
        hipLaunchKernelGGL(strand_nobound_kernel, dim3(g256), dim3(256), 0, stream, n, meta, ctx->strand_dbg);  // every read runs forward first
        ZSW_HIP(ctx, hipGetLastError());
    }
    zsw_error ze = run_score(ctx, against_reference(ctx), &first, rule, {d_score, d_status, d_tier, nullptr, nullptr}, stream);
    if (ze != ZSW_OK) return ze;
    SettleArgs se;
    se.n = n;
    se.meta = meta;
    se.score = d_score;
    se.status = d_status;
    se.strand = d_strand;
    se.list = ws[ST_LIST].as<uint32_t>();
    se.counts = counts;
    se.use_bounds = use_bounds ? 1 : 0;
    se.dbg = ctx->strand_dbg;
    hipLaunchKernelGGL(strand_settle_kernel, dim3(g256), dim3(256), 0, stream, se);
    ZSW_HIP(ctx, hipGetLastError());
    uint32_t n2 = 0;  // the one synchronisation of the call: how many reads need their other strand
    ZSW_HIP(ctx, hipMemcpyAsync(&n2, counts + STC_BOTH, 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    if (n2 == 0) return ZSW_OK;
    if (n2 > n) return fail(ctx, ZSW_ERR_HIP, "strand pass: more unsettled reads than reads");
    // the other strand of the listed reads, compacted
    ZSW_HIP(ctx, ws[ST_SECOND].ensure(total + 16));
    ZSW_HIP(ctx, ws[ST_S2_SCORE].ensure((size_t)n2 * 4 + 4));
    ZSW_HIP(ctx, ws[ST_S2_STATUS].ensure((size_t)n2 + 4));
    ZSW_HIP(ctx, ws[ST_S2_TIER].ensure((size_t)n2 + 4));
    OrientArgs o{};
    o.src = reads->bases;
    o.src_off = reads->offsets;
    o.fixed_len = L;
    o.items = ws[ST_LIST].as<uint32_t>();
    o.n_items = n2;
    o.dst = ws[ST_SECOND].as<uint8_t>();
    o.meta = meta;
    o.flip = 1;
    o.ct = ct;
    zsw_batch second = *reads;
    second.bases = ws[ST_SECOND].as<uint8_t>();
    second.n_reads = n2;
    second.offsets = nullptr;
    if (reads->offsets) {
        ZSW_HIP(ctx, ws[ST_SECOND_OFF].ensure(2 * ((size_t)n2 + 1) * 8));
        uint64_t* lens = ws[ST_SECOND_OFF].as<uint64_t>();
        uint64_t* offs = lens + n2 + 1;
        hipLaunchKernelGGL(strand_lengths_kernel, dim3((n2 + 256) / 256), dim3(256), 0, stream, reads->offsets, o.items, n2, lens);
        ZSW_HIP(ctx, hipGetLastError());
        size_t temp_bytes = 0;
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, lens, offs, (int)(n2 + 1), stream));
        ZSW_HIP(ctx, ws[ST_SCAN_TMP].ensure(temp_bytes + 16));
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[ST_SCAN_TMP].p, temp_bytes, lens, offs, (int)(n2 + 1), stream));
        o.dst_off = offs;
        second.offsets = offs;
    }
    ZSW_HIP(ctx, launch_orient(o, stream));
    ze = run_score(ctx, against_reference(ctx), &second, rule, {ws[ST_S2_SCORE].as<uint32_t>(), ws[ST_S2_STATUS].as<uint8_t>(), ws[ST_S2_TIER].as<uint8_t>(), nullptr, nullptr}, stream);
    if (ze != ZSW_OK) return ze;
    MergeArgs m;
    m.n2 = n2;
    m.list = o.items;
    m.score2 = ws[ST_S2_SCORE].as<uint32_t>();
    m.status2 = ws[ST_S2_STATUS].as<uint8_t>();
    m.tier2 = ws[ST_S2_TIER].as<uint8_t>();
    m.score = d_score;
    m.status = d_status;
    m.tier = d_tier;
    m.strand = d_strand;
    m.counts = counts;
    hipLaunchKernelGGL(strand_merge_kernel, dim3((n2 + 255) / 256), dim3(256), 0, stream, m);
    ZSW_HIP(ctx, hipGetLastError());
    return ZSW_OK;
}

// bytes of a batch's bases (a ragged device batch: its last offset comes back from the device)
zsw_error batch_bytes(zsw_context* ctx, const zsw_batch* reads, hipStream_t stream, size_t* total) {
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

// zsw_score_strands_batch_from for host and device batches
zsw_error score_strands(zsw_context* ctx, const zsw_batch* reads, const ResultRule& rule, uint32_t* out_score, uint8_t* out_status, uint8_t* out_tier,
                        uint8_t* out_strand, hipStream_t stream) {
    if (!reads->offsets && reads->fixed_len == 0 && reads->n_reads) return fail(ctx, ZSW_ERR_EMPTY_SEQUENCE, "fixed-length batch of empty reads");
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    size_t total = 0;
    zsw_error ze = batch_bytes(ctx, reads, stream, &total);
    if (ze != ZSW_OK) return ze;
    if (reads->mem != ZSW_MEM_HOST) return score_strands_device(ctx, reads, total, rule, out_score, out_status, out_tier, out_strand, stream);
    // a host batch: the bases cross once, both score passes and the kernels between them run on the device copy
    const size_t n = reads->n_reads;
    DevBuf* ws = ctx->st_ws;
    ZSW_HIP(ctx, ws[ST_IN].ensure(total + 16));
    ZSW_HIP(ctx, ws[ST_OUT_SCORE].ensure(n * 4 + 4));
    ZSW_HIP(ctx, ws[ST_OUT_STATUS].ensure(n + 4));
    ZSW_HIP(ctx, ws[ST_OUT_TIER].ensure(n + 4));
    ZSW_HIP(ctx, ws[ST_OUT_STRAND].ensure(n + 4));
    if (total) ZSW_HIP(ctx, hipMemcpyAsync(ws[ST_IN].p, reads->bases, total, hipMemcpyHostToDevice, stream));
    zsw_batch dev = *reads;
    dev.mem = ZSW_MEM_DEVICE;
    dev.bases = ws[ST_IN].as<uint8_t>();
    if (reads->offsets) {
        ZSW_HIP(ctx, ws[ST_IN_OFF].ensure((n + 1) * 8));
        ZSW_HIP(ctx, hipMemcpyAsync(ws[ST_IN_OFF].p, reads->offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
        dev.offsets = ws[ST_IN_OFF].as<uint64_t>();
    }
    ze = score_strands_device(ctx, &dev, total, rule, ws[ST_OUT_SCORE].as<uint32_t>(), ws[ST_OUT_STATUS].as<uint8_t>(),
                              out_tier ? ws[ST_OUT_TIER].as<uint8_t>() : nullptr, ws[ST_OUT_STRAND].as<uint8_t>(), stream);
    if (ze != ZSW_OK || n == 0) return ze;
    ZSW_HIP(ctx, hipMemcpyAsync(out_score, ws[ST_OUT_SCORE].p, n * 4, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipMemcpyAsync(out_status, ws[ST_OUT_STATUS].p, n, hipMemcpyDeviceToHost, stream));
    if (out_tier) ZSW_HIP(ctx, hipMemcpyAsync(out_tier, ws[ST_OUT_TIER].p, n, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipMemcpyAsync(out_strand, ws[ST_OUT_STRAND].p, n, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    return ZSW_OK;
}

// the oriented copy of a host batch, on the host
void orient_host(const zsw_batch* reads, const uint8_t* strand, const ComplementTable& ct, uint8_t* out) {
    for (uint64_t i = 0; i < reads->n_reads; ++i) {
        const uint64_t off = reads->offsets ? reads->offsets[i] : i * reads->fixed_len;
        const uint64_t len = reads->offsets ? reads->offsets[i + 1] - off : reads->fixed_len;
        const uint8_t* s = reads->bases + off;
        uint8_t* d = out + off;
        if (strand[i])
            for (uint64_t c = 0; c < len; ++c) d[c] = ct.t[s[len - 1 - c]];
        else
            memcpy(d, s, len);
    }
}

}  // namespace

extern "C" {

zsw_error zsw_set_complement(zsw_context* ctx, const uint8_t* table) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (table) ctx->complement.assign(table, table + 256);
    else ctx->complement.clear();
    return ZSW_OK;
}

zsw_error zsw_score_strands_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, uint32_t* out_score,
                                       uint8_t* out_status, uint8_t* out_tier, uint8_t* out_strand, void* stream) {
    DeviceGuard device_guard(ctx);
    if (zsw_error ze = min_score_unsupported(ctx, "zsw_score_strands_batch_from"); ze != ZSW_OK) return ze;
    if (zsw_error ze = check_strand_batch(ctx, reads, true); ze != ZSW_OK) return ze;
    if (!out_score || !out_status || !out_strand) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    ResultRule rule;
    if (zsw_error ze = rule_cascade(ctx, from_width, preset_bits, &rule); ze != ZSW_OK) return ze;
    return score_strands(ctx, reads, rule, out_score, out_status, out_tier, out_strand, (hipStream_t)stream);
}

zsw_error zsw_orient_batch(zsw_context* ctx, const zsw_batch* reads, const uint8_t* strand, uint8_t* out_bases, void* stream_) {
    DeviceGuard device_guard(ctx);
    if (zsw_error ze = check_strand_batch(ctx, reads, false); ze != ZSW_OK) return ze;
    if (reads->n_reads && (!strand || !out_bases)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (reads->n_reads == 0) return ZSW_OK;
    const ComplementTable ct = complement_of(ctx);
    if (reads->mem == ZSW_MEM_HOST) {
        orient_host(reads, strand, ct, out_bases);
        return ZSW_OK;
    }
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    OrientArgs o{};
    o.src = reads->bases;
    o.src_off = reads->offsets;
    o.fixed_len = reads->fixed_len;
    o.n_items = (uint32_t)reads->n_reads;
    o.dst = out_bases;
    o.strand = strand;
    o.ct = ct;
    ZSW_HIP(ctx, launch_orient(o, (hipStream_t)stream_));
    return ZSW_OK;
}

zsw_error zsw_align_3pass_strands_batch_from(zsw_context* ctx, const zsw_batch* reads, int from_width, int preset_bits, int invert,
                                             zsw_alignment* out_aln, uint8_t* out_status, uint8_t* out_tier, uint8_t* out_strand, uint32_t* out_inc,
                                             uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream_) {
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (zsw_error ze = min_score_unsupported(ctx, "zsw_align_3pass_strands_batch_from"); ze != ZSW_OK) return ze;
    if (zsw_error ze = check_strand_batch(ctx, reads, true); ze != ZSW_OK) return ze;
    if (!out_aln || !out_status || !out_strand || !out_n_ciglets || (ciglet_cap && (!out_inc || !out_op))) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    ResultRule rule;
    if (zsw_error ze = rule_cascade(ctx, from_width, preset_bits, &rule); ze != ZSW_OK) return ze;
    const size_t n = reads->n_reads;
    zsw_batch oriented = *reads;
    // the strand decision by the score call (its scores are not kept: the alignment of the chosen orientation reports its own)
    if (reads->mem == ZSW_MEM_HOST) {
        std::vector<uint32_t> score(n + 1);
        zsw_error ze = score_strands(ctx, reads, rule, score.data(), out_status, nullptr, out_strand, stream);
        if (ze != ZSW_OK) return ze;
        const size_t total = reads->offsets ? (size_t)reads->offsets[n] : n * reads->fixed_len;
        ctx->h_orient.resize(total + 1);
        orient_host(reads, out_strand, complement_of(ctx), ctx->h_orient.data());
        oriented.bases = ctx->h_orient.data();
    } else {
        if (!reads->offsets && reads->fixed_len == 0 && n) return fail(ctx, ZSW_ERR_EMPTY_SEQUENCE, "fixed-length batch of empty reads");
        ZSW_HIP(ctx, hipSetDevice(ctx->device));
        size_t total = 0;
        zsw_error ze = batch_bytes(ctx, reads, stream, &total);
        if (ze != ZSW_OK) return ze;
        DevBuf* ws = ctx->st_ws;
        ZSW_HIP(ctx, ws[ST_OUT_SCORE].ensure(n * 4 + 4));
        ZSW_HIP(ctx, ws[ST_OUT_STATUS].ensure(n + 4));
        ZSW_HIP(ctx, ws[ST_ORIENT_FINAL].ensure(total + 16));
        ze = score_strands_device(ctx, reads, total, rule, ws[ST_OUT_SCORE].as<uint32_t>(), ws[ST_OUT_STATUS].as<uint8_t>(), nullptr, out_strand, stream);
        if (ze != ZSW_OK) return ze;
        OrientArgs o{};
        o.src = reads->bases;
        o.src_off = reads->offsets;
        o.fixed_len = reads->fixed_len;
        o.n_items = (uint32_t)n;
        o.dst = ws[ST_ORIENT_FINAL].as<uint8_t>();
        o.strand = out_strand;
        o.ct = complement_of(ctx);
        ZSW_HIP(ctx, launch_orient(o, stream));
        oriented.bases = ws[ST_ORIENT_FINAL].as<uint8_t>();
    }
    // one alignment run, on the oriented batch
    return run_threepass(ctx, &oriented, rule, invert, {out_aln, out_status, out_tier, out_inc, out_op, ciglet_cap, out_n_ciglets}, stream_);
}

zsw_error zsw_strand_counts(zsw_context* ctx, uint64_t* out) {
    DeviceGuard device_guard(ctx);
    if (!ctx || !out) return ZSW_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < STC_N; ++k) out[k] = 0;
    if (!ctx->st_ws[ST_COUNTS].p) return ZSW_OK;
    uint32_t c[STC_N];
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    ZSW_HIP(ctx, hipDeviceSynchronize());
    ZSW_HIP(ctx, hipMemcpy(c, ctx->st_ws[ST_COUNTS].p, sizeof(c), hipMemcpyDeviceToHost));
    for (int k = 0; k < STC_N; ++k) out[k] = c[k];
    return ZSW_OK;
}

zsw_error zsw_debug_strand_records(zsw_context* ctx, int32_t* records) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    ctx->strand_dbg = records;
    return ZSW_OK;
}

}  // extern "C"
