// zsw_pileup.hip — zsw_pileup_batch and zsw_consensus_from_counts (include/zoe_sw.h): the records of an alignment call piled up
// over the context's sequence, and the plurality base per site. The rules, the two walks and the difference-array decomposition are
// zsw_pileup.hpp (shared with tests/models/pileup_walk.cpp); this file is the wavefront behind the walks' Io, the launches and the
// entry points.
//
// Three launches: (1) pileup_kernel, one wavefront per alignment as zsw_annotate.hip (PILEUP_G = 64 lanes, PILEUP_WAVES per block,
// blocks striding over the batch): validate() over the ciglets, then count(). Per sweep lane l loads byte l of the read's window and
// looks up the bin of site l; a ballot of "the bins differ" skips the sweep's atomics altogether when no lane has one. The range
// adds are two atomic adds per ciglet by two lanes. For sequences of up to PILEUP_LDS_SITES_MAX sites the accumulators (Diff per
// site) and the sequence's bins live in the block's LDS and are added to the global workspace when the block ends, flat over their
// dwords: consecutive lanes, consecutive words. Beyond that every add is a global atomic on the workspace. The sparse
// counts[site][bin] adds and the insertion table go to the caller's tables directly. (2) hipcub's inclusive scan of the workspace
// under pile::combine. (3) resolve_kernel, one thread per site: resolve_site() into the caller's table; the pile-up launch is
// complete by then, plain adds do.
//
// Records and ciglets are caller memory: record_ok() and validate() (64-bit) come before every load or add that an index derived
// from them feeds; a malformed record is a count in *out_n_bad.
#include <hipcub/hipcub.hpp>

#include "zsw_context.hpp"
#include "zsw_pileup.hpp"
#include "zsw_wave.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::pile;
using namespace zsw::wave;

static_assert(sizeof(zsw_site_counts) == 32 && sizeof(zsw_site_insertions) == 8, "the tables' entries");
static_assert(sizeof(zsw_alignment) == sizeof(Rec), "Rec mirrors zsw_alignment");
static_assert(sizeof(Diff) == 16, "Diff is four dwords");
static_assert((int)ZSW_PILEUP_CLEAR == F_CLEAR && (int)ZSW_ANNOTATE_READ_IS_REF == F_READ_IS_REF && (int)ZSW_ANNOTATE_SHARED == F_SHARED, "flags");
static_assert((int)ZSW_CONSENSUS_KEEP_UNCOVERED == K_KEEP_UNCOVERED, "flags");

namespace {

enum { PU_DIFF = 0, PU_NBAD, PU_SCAN_TMP, PU_BASES, PU_OFFSETS, PU_ALN, PU_STATUS, PU_INC, PU_OP, PU_COUNTS, PU_INS, PU_FALLBACK, PU_SEQ, PU_N };

struct PileArgs {
    const uint8_t* bases;
    const uint64_t* offsets;  // null: fixed_len
    uint32_t fixed_len;
    uint32_t n;
    const uint8_t* seq;       // the context's sequence the flags name
    uint32_t seq_len;
    int flags;
    const zsw_alignment* aln;
    const uint8_t* status;
    const uint32_t* inc;
    const uint8_t* op;
    uint64_t n_ciglets;
    uint32_t* diff;           // the workspace: (seq_len + 1) Diff, flat
    uint32_t* counts;         // seq_len * 8
    uint32_t* ins;            // (seq_len + 1) * 2, or null
    unsigned long long* n_bad;
};

constexpr uint32_t PILEUP_BLOCK = 64 * PILEUP_WAVES;
constexpr uint32_t LDS_TABLE = 256;  // bin_of() of every byte

// LDS_ACC: acc and seq_bins point into the block's LDS; else acc is the global workspace and the sequence's bytes are read through L2
template <bool LDS_ACC>
struct WaveIo {
    int lane;
    const uint8_t* read;
    const uint8_t* seq;
    const uint8_t* seq_bins;
    const uint8_t* bin_tab;
    uint32_t* acc;
    uint32_t* counts;
    uint32_t* ins;
    const uint32_t* inc;  // the record's ciglets
    const uint8_t* op;
    uint32_t n_ciglets;
    uint32_t c_inc = 0, c_op = 0;  // ciglet (k & ~63) + lane

    __device__ __forceinline__ void ciglet(uint32_t k, uint32_t* i, uint8_t* o) {
        const uint32_t slot = k & (PILEUP_G - 1);
        if (slot == 0) {  // the next PILEUP_G ciglets, lane l loads ciglet k + l
            c_inc = 0;
            c_op = 0;
            if ((uint64_t)k + lane < n_ciglets) {
                c_inc = inc[k + lane];
                c_op = op[k + lane];
            }
        }
        *i = uni((uint32_t)__shfl((int)c_inc, (int)slot, 64));
        *o = (uint8_t)uni((uint32_t)__shfl((int)c_op, (int)slot, 64));
    }
    __device__ __forceinline__ void range(int which, uint64_t site, uint32_t n) {
        if (lane < 2) atomicAdd(&acc[(site + (lane ? n : 0u)) * D_FIELDS + which], lane ? 0xffffffffu : 1u);
    }
    __device__ __forceinline__ void columns(uint64_t site, uint64_t rd, int nv) {
        int b = 0;
        bool differ = false;
        if (lane < nv) {
            b = bin_tab[read[rd + lane]];
            const int e = LDS_ACC ? seq_bins[site + lane] : bin_tab[seq[site + lane]];
            differ = b != e;
        }
        if (__ballot(differ) == 0) return;
        if (differ) {
            atomicAdd(&acc[(site + lane) * D_FIELDS + D_MISS], 1u);
            atomicAdd(&counts[(site + lane) * N_BINS + b], 1u);
        }
    }
    __device__ __forceinline__ void insertion(uint64_t p, uint32_t n) {
        if (lane < 2) atomicAdd(&ins[p * 2 + lane], lane ? n : 1u);
    }
};

template <bool LDS_ACC>
__global__ __launch_bounds__(PILEUP_BLOCK) void pileup_kernel(PileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* bin_tab = lds;
    uint32_t* acc = a.diff;
    const uint8_t* seq_bins = nullptr;
    const uint32_t n_acc = (a.seq_len + 1) * D_FIELDS;  // seq_len <= PILEUP_LDS_SITES_MAX where it is used
    if (threadIdx.x < 256) bin_tab[threadIdx.x] = (uint8_t)bin_of((uint8_t)threadIdx.x);
    if (LDS_ACC) {
        acc = reinterpret_cast<uint32_t*>(lds + LDS_TABLE);
        uint8_t* sb = lds + LDS_TABLE + n_acc * 4;
        for (uint32_t k = threadIdx.x; k < n_acc; k += PILEUP_BLOCK) acc[k] = 0;
        for (uint32_t k = threadIdx.x; k < a.seq_len; k += PILEUP_BLOCK) sb[k] = (uint8_t)bin_of(a.seq[k]);
        seq_bins = sb;
    }
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const bool swap = (a.flags & F_READ_IS_REF) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * PILEUP_WAVES;
    for (uint64_t i = (uint64_t)blockIdx.x * PILEUP_WAVES + wave; i < a.n; i += stride) {
        if (uni((uint32_t)a.status[i]) != ZSW_STATUS_SOME) continue;
        const zsw_alignment in = a.aln[i];
        const uint64_t off = a.offsets ? uni(a.offsets[i]) : i * a.fixed_len;
        const uint32_t len = a.offsets ? (uint32_t)(uni(a.offsets[i + 1]) - off) : a.fixed_len;
        const Rec rec{uni(in.score), uni(in.ref_start), uni(in.ref_end), uni(in.query_start), uni(in.query_end), uni(in.ref_len), uni(in.query_len),
                      uni(in.n_ciglets), uni(in.ciglet_offset)};
        bool ok = ann::record_ok(rec, a.n_ciglets, swap ? len : a.seq_len, swap ? a.seq_len : len);
        WaveIo<LDS_ACC> io;
        if (ok) {
            io.lane = lane;
            io.read = a.bases + off;
            io.seq = a.seq;
            io.seq_bins = seq_bins;
            io.bin_tab = bin_tab;
            io.acc = acc;
            io.counts = a.counts;
            io.ins = a.ins;
            io.inc = a.inc + rec.ciglet_offset;
            io.op = a.op + rec.ciglet_offset;
            io.n_ciglets = rec.n_ciglets;
            ok = validate(io, rec);
        }
        if (!ok) {
            if (lane == 0) atomicAdd(a.n_bad, 1ull);
            continue;
        }
        count(io, rec, swap, a.ins != nullptr);
    }
    if (LDS_ACC) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < n_acc; k += PILEUP_BLOCK) {
            const uint32_t v = acc[k];
            if (v) atomicAdd(&a.diff[k], v);
        }
    }
}

struct CombineOp {
    __host__ __device__ __forceinline__ Diff operator()(const Diff& x, const Diff& y) const { return combine(x, y); }
};

__global__ __launch_bounds__(256) void resolve_kernel(const Diff* sums, const uint8_t* seq, uint32_t len, uint32_t* counts) {
    const uint32_t pos = blockIdx.x * 256u + threadIdx.x;
    if (pos >= len) return;
    const Diff d = sums[pos];
    uint32_t add[N_BINS] = {};
    resolve_site(add, d, bin_of(seq[pos]));
    uint32_t* c = counts + (size_t)pos * N_BINS;
#pragma unroll
    for (int b = 0; b < N_BINS; ++b) c[b] += add[b];
}

__global__ __launch_bounds__(256) void consensus_kernel(const uint32_t* counts, uint64_t len, int flags, const uint8_t* fallback, uint8_t* out) {
    const uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (pos >= len) return;
    uint32_t bins[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) bins[b] = counts[pos * N_BINS + b];
    out[pos] = consensus_byte(bins, flags, (flags & K_KEEP_UNCOVERED) ? fallback[pos] : (uint8_t)0);
}

uint32_t pileup_lds_bytes(uint32_t seq_len) { return LDS_TABLE + (seq_len + 1) * (uint32_t)sizeof(Diff) + ((seq_len + 15u) & ~15u); }

hipError_t launch_pileup(const zsw_context* ctx, const PileArgs& a, hipStream_t stream) {
    const bool lds_acc = a.seq_len <= PILEUP_LDS_SITES_MAX;
    const uint64_t want = ((uint64_t)a.n + PILEUP_WAVES - 1) / PILEUP_WAVES;
    if (lds_acc) {  // a block pays for zeroing and flushing its accumulators: no more blocks than stay resident
        const uint32_t lds = pileup_lds_bytes(a.seq_len);
        const uint64_t resident = std::max<uint64_t>(1, std::min<uint64_t>(4, (160u * 1024u) / lds));
        const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)ctx->cu_count * resident);
        if (lds > 48 * 1024) {  // above the default dynamic-LDS limit: raise it (per device, as zsw_align.hip)
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pileup_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)pileup_lds_bytes(PILEUP_LDS_SITES_MAX));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((pileup_kernel<true>), dim3(grid), dim3(PILEUP_BLOCK), lds, stream, a);
    } else {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)ctx->cu_count * 4);
        hipLaunchKernelGGL((pileup_kernel<false>), dim3(grid), dim3(PILEUP_BLOCK), LDS_TABLE, stream, a);
    }
    return hipGetLastError();
}

}  // namespace

extern "C" zsw_error zsw_pileup_batch(zsw_context* ctx, const zsw_batch* reads, int flags, const zsw_alignment* aln, const uint8_t* status,
                                      const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, void* counts_, void* ins_, uint64_t* out_n_bad,
                                      void* stream_) {
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    zsw_site_counts* counts = static_cast<zsw_site_counts*>(counts_);
    zsw_site_insertions* ins = static_cast<zsw_site_insertions*>(ins_);
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (!reads || !out_n_bad) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~F_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown pile-up flag");
    if (reads->encoding == ZSW_ENCODING_PACKED4) return fail(ctx, ZSW_ERR_UNSUPPORTED, "zsw_pileup_batch takes ZSW_ENCODING_BYTES (it bins the reads' bytes)");
    if (reads->encoding != ZSW_ENCODING_BYTES) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.encoding");
    if (reads->mem != ZSW_MEM_HOST && reads->mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.mem");
    const bool shared = (flags & F_SHARED) != 0;
    if (shared ? !ctx->pseq_set : !ctx->reference_set) return fail(ctx, ZSW_ERR_NOT_CONFIGURED, shared ? "profile sequence not set" : "reference not set");
    const size_t seq_len = shared ? ctx->pseq_len : ctx->ref_len;
    if (seq_len >= 0x7fffffffull) return fail(ctx, ZSW_ERR_UNSUPPORTED, "sequences of 2^31 - 1 bases or more");
    const uint64_t n = reads->n_reads;
    if (n > 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_reads > 2^31-1 per call");
    if (seq_len && !counts) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (n && (!reads->bases || !aln || !status)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (n_ciglets && (!inc || !op)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null ciglet arrays");
    const bool host = reads->mem == ZSW_MEM_HOST;
    if (host && reads->offsets)
        for (uint64_t i = 0; i < n; ++i)
            if (reads->offsets[i + 1] < reads->offsets[i]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
    const size_t counts_bytes = seq_len * sizeof(zsw_site_counts), ins_bytes = ins ? (seq_len + 1) * sizeof(zsw_site_insertions) : 0;
    {  // no table over an input array (the bases of a ragged device batch: their size is not known here) or over the other table
        const void* outs[2] = {counts, ins};
        const size_t out_bytes[2] = {counts_bytes, ins_bytes};
        const void* inputs[4] = {aln, status, inc, op};
        const size_t in_bytes[4] = {(size_t)n * sizeof(zsw_alignment), (size_t)n, (size_t)n_ciglets * 4, (size_t)n_ciglets};
        for (int o = 0; o < 2; ++o) {
            for (int k = 0; k < 4; ++k)
                if (overlaps(outs[o], out_bytes[o], inputs[k], in_bytes[k])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a table overlaps an input array");
            if (n && (!reads->offsets || host) && overlaps(outs[o], out_bytes[o], reads->bases, reads->offsets ? (size_t)reads->offsets[n] : (size_t)n * reads->fixed_len))
                return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a table overlaps the reads");
        }
        if (overlaps(counts, counts_bytes, ins, ins_bytes)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "the tables overlap");
    }
    *out_n_bad = 0;
    const bool clear = (flags & F_CLEAR) != 0;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        if (clear && host) {
            if (counts_bytes) memset(counts, 0, counts_bytes);
            if (ins_bytes) memset(ins, 0, ins_bytes);
        } else if (clear) {
            if (counts_bytes) ZSW_HIP(ctx, hipMemsetAsync(counts, 0, counts_bytes, stream));
            if (ins_bytes) ZSW_HIP(ctx, hipMemsetAsync(ins, 0, ins_bytes, stream));
        }
        return ZSW_OK;
    }
    DevBuf* ws = ctx->pu_ws;
    static_assert(PU_N <= sizeof(ctx->pu_ws) / sizeof(ctx->pu_ws[0]), "zsw_context::pu_ws holds every buffer");
    PileArgs a{};
    a.bases = reads->bases;
    a.offsets = reads->offsets;
    a.fixed_len = reads->fixed_len;
    a.n = (uint32_t)n;
    a.seq = shared ? ctx->d_pseq.as<uint8_t>() : ctx->d_ref.as<uint8_t>();
    a.seq_len = (uint32_t)seq_len;
    a.flags = flags;
    a.aln = aln;
    a.status = status;
    a.inc = inc;
    a.op = op;
    a.n_ciglets = n_ciglets;
    a.counts = reinterpret_cast<uint32_t*>(counts);
    a.ins = reinterpret_cast<uint32_t*>(ins);
    const size_t diff_bytes = (seq_len + 1) * sizeof(Diff);
    ZSW_HIP(ctx, ws[PU_DIFF].ensure(diff_bytes));
    ZSW_HIP(ctx, ws[PU_NBAD].ensure(8));
    a.diff = ws[PU_DIFF].as<uint32_t>();
    a.n_bad = ws[PU_NBAD].as<unsigned long long>();
    ZSW_HIP(ctx, hipMemsetAsync(a.diff, 0, diff_bytes, stream));
    ZSW_HIP(ctx, hipMemsetAsync(a.n_bad, 0, 8, stream));
    if (host) {  // everything crosses once, the tables both ways; the call returns when they are back
        const size_t total = reads->offsets ? (size_t)reads->offsets[n] : (size_t)n * reads->fixed_len;
        if (zsw_error up = stage_up_records(ctx, ws + PU_BASES, reads->bases, total, &a, stream)) return up;
        ZSW_HIP(ctx, ws[PU_COUNTS].ensure(counts_bytes + 32));
        if (ins) ZSW_HIP(ctx, ws[PU_INS].ensure(ins_bytes));
        if (!clear) {
            if (counts_bytes) ZSW_HIP(ctx, hipMemcpyAsync(ws[PU_COUNTS].p, counts, counts_bytes, hipMemcpyHostToDevice, stream));
            if (ins) ZSW_HIP(ctx, hipMemcpyAsync(ws[PU_INS].p, ins, ins_bytes, hipMemcpyHostToDevice, stream));
        }
        a.counts = ws[PU_COUNTS].as<uint32_t>();
        if (ins) a.ins = ws[PU_INS].as<uint32_t>();
    }
    if (clear) {
        if (counts_bytes) ZSW_HIP(ctx, hipMemsetAsync(a.counts, 0, counts_bytes, stream));
        if (a.ins) ZSW_HIP(ctx, hipMemsetAsync(a.ins, 0, ins_bytes, stream));
    }
    hipError_t e = launch_pileup(ctx, a, stream);
    if (e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, "pile-up", e);
    Diff* d = ws[PU_DIFF].as<Diff>();
    size_t temp_bytes = 0;
    ZSW_HIP(ctx, hipcub::DeviceScan::InclusiveScan(nullptr, temp_bytes, d, d, CombineOp(), (int)(seq_len + 1), stream));
    ZSW_HIP(ctx, ws[PU_SCAN_TMP].ensure(temp_bytes + 16));
    ZSW_HIP(ctx, hipcub::DeviceScan::InclusiveScan(ws[PU_SCAN_TMP].p, temp_bytes, d, d, CombineOp(), (int)(seq_len + 1), stream));
    if (seq_len) {
        hipLaunchKernelGGL(resolve_kernel, dim3((uint32_t)((seq_len + 255) / 256)), dim3(256), 0, stream, d, a.seq, a.seq_len, a.counts);
        ZSW_HIP(ctx, hipGetLastError());
    }
    uint64_t n_bad = 0;  // the one synchronisation of a device call
    ZSW_HIP(ctx, hipMemcpyAsync(&n_bad, a.n_bad, 8, hipMemcpyDeviceToHost, stream));
    if (host) {
        if (counts_bytes) ZSW_HIP(ctx, hipMemcpyAsync(counts, a.counts, counts_bytes, hipMemcpyDeviceToHost, stream));
        if (ins) ZSW_HIP(ctx, hipMemcpyAsync(ins, a.ins, ins_bytes, hipMemcpyDeviceToHost, stream));
    }
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    *out_n_bad = n_bad;
    return ZSW_OK;
}

extern "C" zsw_error zsw_consensus_from_counts(zsw_context* ctx, const void* counts_, uint64_t len, zsw_mem mem, int flags, const uint8_t* fallback,
                                               uint8_t* out_seq, void* stream_) {
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (flags & ~K_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown consensus flag");
    if (mem != ZSW_MEM_HOST && mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_mem");
    if (len >= 0x7fffffffull) return fail(ctx, ZSW_ERR_UNSUPPORTED, "sequences of 2^31 - 1 bases or more");
    const bool keep = (flags & K_KEEP_UNCOVERED) != 0;
    if (len && (!counts_ || !out_seq || (keep && !fallback))) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (overlaps(out_seq, len, counts_, len * sizeof(zsw_site_counts)) || (keep && overlaps(out_seq, len, fallback, len)))
        return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "out_seq overlaps an input array");
    if (len == 0) return ZSW_OK;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_counts = static_cast<const uint32_t*>(counts_);
    const uint8_t* d_fb = fallback;
    uint8_t* d_out = out_seq;
    const bool host = mem == ZSW_MEM_HOST;
    if (host) {
        DevBuf* ws = ctx->pu_ws;
        ZSW_HIP(ctx, ws[PU_COUNTS].ensure(len * sizeof(zsw_site_counts)));
        ZSW_HIP(ctx, ws[PU_SEQ].ensure(len));
        ZSW_HIP(ctx, hipMemcpyAsync(ws[PU_COUNTS].p, counts_, len * sizeof(zsw_site_counts), hipMemcpyHostToDevice, stream));
        if (keep) {
            ZSW_HIP(ctx, ws[PU_FALLBACK].ensure(len));
            ZSW_HIP(ctx, hipMemcpyAsync(ws[PU_FALLBACK].p, fallback, len, hipMemcpyHostToDevice, stream));
            d_fb = ws[PU_FALLBACK].as<uint8_t>();
        }
        d_counts = ws[PU_COUNTS].as<uint32_t>();
        d_out = ws[PU_SEQ].as<uint8_t>();
    }
    hipLaunchKernelGGL(consensus_kernel, dim3((uint32_t)((len + 255) / 256)), dim3(256), 0, stream, d_counts, len, flags, d_fb, d_out);
    ZSW_HIP(ctx, hipGetLastError());
    if (host) {
        ZSW_HIP(ctx, hipMemcpyAsync(out_seq, d_out, len, hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
