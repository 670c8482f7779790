// zsw_annotate.hip — zsw_annotate_batch (include/zoe_sw.h): =/X CIGARs, edit counts and sw_score_from_path for the records of an
// alignment call, in one pass over each CIGAR beside its two sequences. The rules and the walk are zsw_annotate.hpp (shared with
// tests/models/annotate_walk.cpp); this file is the wavefront behind the walk's Io, the launches and the entry point.
//
// One wavefront per alignment (ANN_G = 64 lanes), ANN_WAVES per block, blocks striding over the batch. Per sweep lane l loads byte l
// of the read's and of the context sequence's window — consecutive lanes, consecutive bytes, as strand_orient_kernel —, a ballot
// makes the match mask, and the =/X run boundaries, their places and their lengths are bit operations on that mask: every run of
// a sweep is written by the lane it starts at. The record, its ciglets and the walk's cursors are wavefront-uniform (uni(), zsw_wave.hpp). The context's
// sequence, the index map and the weights are staged in LDS once per block (sequences beyond ANN_LDS_SEQ_MAX bytes: through L2);
// a read's bases and ciglets pass through the wavefront's own LDS area, loaded together while the next read's record is in flight.
//
// Records and ciglets are caller memory: record_ok() and the walk's own range checks (64-bit) come before every load that an
// index derived from them feeds; a malformed record is a ZSW_PATH_* status. The verbose CIGAR has a variable length: a count
// launch, hipcub's exclusive sum, a write launch that walks again. Without out_aln: the count launch alone, nothing else.
#include <hipcub/hipcub.hpp>

#include "zsw_annotate.hpp"
#include "zsw_context.hpp"
#include "zsw_wave.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::ann;
using namespace zsw::wave;

static_assert(sizeof(zsw_alignment_stats) == 32 && sizeof(Stats) == 32, "zsw_alignment_stats is 32 bytes");
static_assert(sizeof(zsw_alignment) == sizeof(Rec), "Rec mirrors zsw_alignment");

namespace {

enum { AN_BASES = 0, AN_OFFSETS, AN_ALN, AN_STATUS, AN_INC, AN_OP, AN_STATS, AN_OUT_ALN, AN_OUT_INC, AN_OUT_OP, AN_COUNTS, AN_STARTS, AN_SCAN_TMP, AN_N };

struct AnnArgs {
    const uint8_t* bases;
    const uint64_t* offsets;  // null: fixed_len
    uint32_t fixed_len;
    uint32_t n;
    const ScoringDev* sc;
    const uint8_t* seq;       // the context's sequence the flags name
    uint32_t seq_len;
    int flags;
    const zsw_alignment* aln;
    const uint8_t* status;
    const uint32_t* inc;
    const uint8_t* op;
    uint64_t n_ciglets;
    zsw_alignment_stats* stats;  // count launch: written; write launch: read
    uint64_t* counts;            // count launch: verbose ciglets per read (null: not wanted)
    const uint64_t* starts;      // write launch: their exclusive sum, n + 1 entries
    zsw_alignment* out_aln;
    uint32_t* out_inc;
    uint8_t* out_op;
};

constexpr uint32_t LDS_TABLES = 256 + MAX_S * MAX_S * 4;
constexpr uint32_t ANN_WAVES = 8;  // wavefronts, i.e. alignments in flight, per block: they share one staged copy of the sequence
constexpr uint32_t ANN_BLOCK = 64 * ANN_WAVES;
constexpr uint32_t ANN_READ_LDS = 512;  // bases of a read that go through the wavefront's LDS area (longer reads: from global memory)
constexpr uint32_t WAVE_LDS = ANN_READ_LDS + 4 * ANN_G + ANN_G;  // ... and ANN_G ciglets: inc, op
constexpr uint32_t LDS_FIXED = LDS_TABLES + ANN_WAVES * WAVE_LDS;

struct WaveIo {
    int lane;
    const uint8_t *qseq, *rseq;  // the record's query and reference sequence (read and context sequence, as the flags say)
    bool q_is_read, shared, residues;
    const uint8_t* im;
    const int32_t* w;
    int S;
    const uint32_t* inc;  // the record's ciglets
    const uint8_t* op;
    uint32_t n_ciglets;
    uint32_t* cinc;       // ANN_G of them in LDS: ciglets [k & ~63, ...)
    uint8_t* cop;
    uint32_t* out_inc;    // the read's verbose ciglets
    uint8_t* out_op;
    uint32_t out_n;       // how many the count launch found: no write beyond them
    int32_t sum = 0;

    __device__ __forceinline__ void ciglet(uint32_t k, uint32_t* i, uint8_t* o) const {
        const uint32_t slot = k & (ANN_G - 1);
        if (slot == 0 && k) {  // the next ANN_G ciglets, lane l loads ciglet k + l
            wave_sync();
            if (k + lane < n_ciglets) {
                cinc[lane] = inc[k + lane];
                cop[lane] = op[k + lane];
            }
            wave_sync();
        }
        *i = uni(cinc[slot]);
        *o = (uint8_t)uni((uint32_t)cop[slot]);
    }
    __device__ __forceinline__ uint64_t sweep(uint64_t q, uint64_t r, int nv) {
        bool eq = false;
        if (lane < nv) {
            const uint8_t qb = qseq[q + lane], rb = rseq[r + lane];
            const int qi = im[qb], ri = im[rb];
            eq = residues ? qi == ri : qb == rb;
            const int read_i = q_is_read ? qi : ri, seq_i = q_is_read ? ri : qi;
            sum += shared ? w[read_i * S + seq_i] : w[seq_i * S + read_i];  // row = non-profile residue, column = profile residue
        }
        return __ballot(eq);
    }
    __device__ __forceinline__ int64_t column_score() const {
        int32_t v = sum;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        return (int64_t)(int32_t)uni((uint32_t)v);
    }
    __device__ __forceinline__ void emit_one(uint32_t pos, uint32_t i, uint8_t o) const {
        if (lane == 0 && pos < out_n) {
            out_inc[pos] = i;
            out_op[pos] = o;
        }
    }
    __device__ __forceinline__ void emit_runs(uint64_t starts, uint64_t mask, uint32_t pos) const {
        uint32_t i, rank;
        uint8_t o;
        if (run_of_lane(starts, mask, lane, &i, &o, &rank) && (uint64_t)pos + rank < out_n) {
            out_inc[pos + rank] = i;
            out_op[pos + rank] = o;
        }
    }
};

// EMIT = false: stats (and the number of verbose ciglets) of every read. EMIT = true: out_aln and the verbose ciglets.
// A wavefront's reads follow each other, and what one read waits for is memory latency: its record, then its ciglets, then the
// bases under every sweep. So the record (and status) of the wavefront's NEXT read is loaded before this one is walked; the read's
// bases (up to ANN_READ_LDS of them, one coalesced pass) and its first ANN_G ciglets (lane k loads ciglet k) are loaded together
// into the wavefront's own LDS area, and the walk's sweeps and ciglet look-ups read LDS.
template <bool EMIT, bool STAGED>
__global__ __launch_bounds__(ANN_BLOCK) void annotate_kernel(AnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* im = lds;
    int32_t* w = reinterpret_cast<int32_t*>(lds + 256);
    if (threadIdx.x < 256) im[threadIdx.x] = a.sc->index_map[threadIdx.x];
    const int S = a.sc->S, gap_open = a.sc->gap_open, gap_extend = a.sc->gap_extend;
    for (int k = threadIdx.x; k < S * S; k += ANN_BLOCK) w[k] = a.sc->w[k];
    const uint8_t* seq = a.seq;
    if (STAGED) {
        uint8_t* sseq = lds + LDS_FIXED;
        for (uint32_t k = threadIdx.x; k < a.seq_len; k += ANN_BLOCK) sseq[k] = a.seq[k];
        seq = sseq;
    }
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    uint8_t* rbuf = lds + LDS_TABLES + wave * WAVE_LDS;
    uint32_t* cinc = reinterpret_cast<uint32_t*>(rbuf + ANN_READ_LDS);
    uint8_t* cop = rbuf + ANN_READ_LDS + 4 * ANN_G;
    const bool read_is_ref = (a.flags & F_READ_IS_REF) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * ANN_WAVES;
    uint64_t i = (uint64_t)blockIdx.x * ANN_WAVES + wave;
    if (i >= a.n) return;
    zsw_alignment in = a.aln[i];
    uint8_t in_status = a.status[i];
    for (; i < a.n; i += stride) {
        const uint64_t ni = i + stride < a.n ? i + stride : i;
        const zsw_alignment next = a.aln[ni];
        const uint8_t next_status = a.status[ni];
        const uint64_t off = a.offsets ? uni(a.offsets[i]) : i * a.fixed_len;
        const uint32_t len = a.offsets ? (uint32_t)(uni(a.offsets[i + 1]) - off) : a.fixed_len;
        Rec rec{uni(in.score), uni(in.ref_start), uni(in.ref_end), uni(in.query_start), uni(in.query_end), uni(in.ref_len), uni(in.query_len),
                uni(in.n_ciglets), uni(in.ciglet_offset)};
        const bool ok = record_ok(rec, a.n_ciglets, read_is_ref ? len : a.seq_len, read_is_ref ? a.seq_len : len);
        const uint32_t st = EMIT ? uni(a.stats[i].path_status) : uni((uint32_t)in_status) != ZSW_STATUS_SOME ? P_NO_ALIGNMENT : ok ? P_OK : P_BAD_RECORD;
        uint64_t start0 = 0, start1 = 0;  // EMIT: the read's place among the verbose ciglets
        if (EMIT) {
            start0 = uni(a.starts[i]);
            start1 = uni(a.starts[i + 1]);
        }
        uint32_t nv = 0;
        if (ok && (EMIT ? annotated(st) : st == P_OK)) {
            const uint8_t* rd = a.bases + off;
            const bool in_lds = len <= ANN_READ_LDS;
            uint8_t rb[ANN_READ_LDS / ANN_G];
            uint32_t c_inc = 0;
            uint8_t c_op = 0;
            if (in_lds) {
#pragma unroll
                for (uint32_t j = 0; j < ANN_READ_LDS / ANN_G; ++j) rb[j] = j * ANN_G + lane < len ? rd[j * ANN_G + lane] : 0;
            }
            if ((uint32_t)lane < rec.n_ciglets) {
                c_inc = a.inc[rec.ciglet_offset + lane];
                c_op = a.op[rec.ciglet_offset + lane];
            }
            wave_sync();  // the previous read's look-ups are done
            if (in_lds) {
#pragma unroll
                for (uint32_t j = 0; j < ANN_READ_LDS / ANN_G; ++j)
                    if (j * ANN_G < len) rbuf[j * ANN_G + lane] = rb[j];
                rd = rbuf;
            }
            cinc[lane] = c_inc;
            cop[lane] = c_op;
            wave_sync();
            WaveIo io;
            io.lane = lane;
            io.qseq = read_is_ref ? seq : rd;
            io.rseq = read_is_ref ? rd : seq;
            io.q_is_read = !read_is_ref;
            io.shared = (a.flags & F_SHARED) != 0;
            io.residues = (a.flags & F_MATCH_RESIDUES) != 0;
            io.im = im;
            io.w = w;
            io.S = S;
            io.inc = a.inc + rec.ciglet_offset;
            io.op = a.op + rec.ciglet_offset;
            io.n_ciglets = rec.n_ciglets;
            io.cinc = cinc;
            io.cop = cop;
            io.out_inc = nullptr;
            io.out_op = nullptr;
            io.out_n = 0;
            if (EMIT) {
                io.out_inc = a.out_inc + start0;
                io.out_op = a.out_op + start0;
                io.out_n = (uint32_t)(start1 - start0);
            }
            const Stats s = walk<EMIT>(io, rec, gap_open, gap_extend, &nv);
            if (!EMIT && lane == 0) reinterpret_cast<Stats*>(a.stats)[i] = s;
        } else if (!EMIT && lane == 0) {
            Stats s{};
            s.path_status = st;
            reinterpret_cast<Stats*>(a.stats)[i] = s;
        }
        if (lane == 0) {
            if (!EMIT && a.counts) a.counts[i] = nv;
            if (EMIT) {
                zsw_alignment o = in;
                o.n_ciglets = (uint32_t)(start1 - start0);
                o.ciglet_offset = start0;
                a.out_aln[i] = o;
            }
        }
        in = next;
        in_status = next_status;
    }
}

// blocks of a launch: the reads' share, and for a staged sequence no more than stay resident — a block pays seq_len bytes before
// its first read (three blocks of ANN_WAVES wavefronts per CU at the threshold)
template <bool EMIT>
hipError_t launch_annotate(const zsw_context* ctx, const AnnArgs& a, hipStream_t stream) {
    if (!a.n) return hipSuccess;
    const bool staged = a.seq_len <= ANN_LDS_SEQ_MAX;
    const uint32_t lds = LDS_FIXED + (staged ? ((a.seq_len + 15u) & ~15u) : 0u);
    const uint64_t want = ((uint64_t)a.n + ANN_WAVES - 1) / ANN_WAVES;
    const uint64_t resident = std::max<uint64_t>(1, std::min<uint64_t>(4, (160u * 1024u) / lds));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, staged ? (uint64_t)ctx->cu_count * resident : (uint64_t)1 << 20);
    if (staged) hipLaunchKernelGGL((annotate_kernel<EMIT, true>), dim3(grid), dim3(ANN_BLOCK), lds, stream, a);
    else hipLaunchKernelGGL((annotate_kernel<EMIT, false>), dim3(grid), dim3(ANN_BLOCK), lds, stream, a);
    return hipGetLastError();
}

// the last entry of the counts (the exclusive sum needs n + 1 inputs for the total)
__global__ void annotate_close_counts(uint64_t* counts, uint32_t n) { counts[n] = 0; }

}  // namespace

extern "C" zsw_error zsw_annotate_batch(zsw_context* ctx, const zsw_batch* reads, int flags, const zsw_alignment* aln, const uint8_t* status,
                                        const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, void* out_stats_, zsw_alignment* out_aln,
                                        uint32_t* out_inc, uint8_t* out_op, uint64_t ciglet_cap, uint64_t* out_n_ciglets, void* stream_) {
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    zsw_alignment_stats* out_stats = static_cast<zsw_alignment_stats*>(out_stats_);
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    if (!reads) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~F_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown annotate flag");
    if (reads->encoding == ZSW_ENCODING_PACKED4) return fail(ctx, ZSW_ERR_UNSUPPORTED, "zsw_annotate_batch takes ZSW_ENCODING_BYTES (it compares the reads' bytes)");
    if (reads->encoding != ZSW_ENCODING_BYTES) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.encoding");
    if (reads->mem != ZSW_MEM_HOST && reads->mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.mem");
    const bool shared = (flags & F_SHARED) != 0;
    if (!ctx->scoring_set || (shared ? !ctx->pseq_set : !ctx->reference_set))
        return fail(ctx, ZSW_ERR_NOT_CONFIGURED, shared ? "scoring/profile sequence not set" : "scoring/reference not set");
    const uint64_t n = reads->n_reads;
    if (n > 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_reads > 2^31-1 per call");
    if (n && (!reads->bases || !aln || !status || !out_stats)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (n_ciglets && (!inc || !op)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null ciglet arrays");
    if (out_aln && (!out_n_ciglets || (ciglet_cap && (!out_inc || !out_op)))) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    const bool host = reads->mem == ZSW_MEM_HOST;
    if (host && reads->offsets)
        for (uint64_t i = 0; i < n; ++i)
            if (reads->offsets[i + 1] < reads->offsets[i]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
    {  // no output array over an input array (the bases of a ragged device batch: their size is not known here)
        const void* outs[4] = {out_stats, out_aln, out_aln ? out_inc : nullptr, out_aln ? out_op : nullptr};
        const size_t out_bytes[4] = {(size_t)n * 32, (size_t)n * sizeof(zsw_alignment), (size_t)ciglet_cap * 4, (size_t)ciglet_cap};
        const void* ins[4] = {aln, status, inc, op};
        const size_t in_bytes[4] = {(size_t)n * sizeof(zsw_alignment), (size_t)n, (size_t)n_ciglets * 4, (size_t)n_ciglets};
        for (int o = 0; o < 4; ++o) {
            for (int k = 0; k < 4; ++k)
                if (overlaps(outs[o], out_bytes[o], ins[k], in_bytes[k])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "an output array overlaps an input array");
            if ((!reads->offsets || host) && overlaps(outs[o], out_bytes[o], reads->bases, reads->offsets ? (size_t)reads->offsets[n] : (size_t)n * reads->fixed_len))
                return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "an output array overlaps the reads");
            for (int k = o + 1; k < 4; ++k)
                if (overlaps(outs[o], out_bytes[o], outs[k], out_bytes[k])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "output arrays overlap");
        }
    }
    if (out_n_ciglets) *out_n_ciglets = 0;
    if (n == 0) return ZSW_OK;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->an_ws;
    AnnArgs a{};
    a.bases = reads->bases;
    a.offsets = reads->offsets;
    a.fixed_len = reads->fixed_len;
    a.n = (uint32_t)n;
    a.sc = ctx->d_sc.as<ScoringDev>();
    a.seq = shared ? ctx->d_pseq.as<uint8_t>() : ctx->d_ref.as<uint8_t>();
    const size_t seq_len = shared ? ctx->pseq_len : ctx->ref_len;
    if (seq_len > 0xffffffffull) return fail(ctx, ZSW_ERR_UNSUPPORTED, "sequences of 2^32 bases or more");
    a.seq_len = (uint32_t)seq_len;
    a.flags = flags;
    a.aln = aln;
    a.status = status;
    a.inc = inc;
    a.op = op;
    a.n_ciglets = n_ciglets;
    a.stats = out_stats;
    if (host) {  // everything crosses once; the call returns when the results are back
        const size_t total = reads->offsets ? (size_t)reads->offsets[n] : (size_t)n * reads->fixed_len;
        if (zsw_error up = stage_up_records(ctx, ws + AN_BASES, reads->bases, total, &a, stream)) return up;
        ZSW_HIP(ctx, ws[AN_STATS].ensure(n * 32));
        a.stats = ws[AN_STATS].as<zsw_alignment_stats>();
    }
    if (out_aln) {
        ZSW_HIP(ctx, ws[AN_COUNTS].ensure((n + 1) * 8));
        ZSW_HIP(ctx, ws[AN_STARTS].ensure((n + 1) * 8));
        a.counts = ws[AN_COUNTS].as<uint64_t>();
    }
    hipError_t e = launch_annotate<false>(ctx, a, stream);
    if (e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, "annotate count", e);
    if (!out_aln) {
        if (host) {
            ZSW_HIP(ctx, hipMemcpyAsync(out_stats, a.stats, n * 32, hipMemcpyDeviceToHost, stream));
            ZSW_HIP(ctx, hipStreamSynchronize(stream));
        }
        return ZSW_OK;
    }
    uint64_t* starts = ws[AN_STARTS].as<uint64_t>();
    hipLaunchKernelGGL(annotate_close_counts, dim3(1), dim3(1), 0, stream, a.counts, (uint32_t)n);
    ZSW_HIP(ctx, hipGetLastError());
    size_t temp_bytes = 0;
    ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.counts, starts, (int)(n + 1), stream));
    ZSW_HIP(ctx, ws[AN_SCAN_TMP].ensure(temp_bytes + 16));
    ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[AN_SCAN_TMP].p, temp_bytes, a.counts, starts, (int)(n + 1), stream));
    uint64_t total = 0;  // the one synchronisation of a device call
    ZSW_HIP(ctx, hipMemcpyAsync(&total, starts + n, 8, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));
    *out_n_ciglets = total;
    if (total > ciglet_cap) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "ciglet capacity too small; required size returned");
    a.counts = nullptr;
    a.starts = starts;
    a.out_aln = out_aln;
    a.out_inc = out_inc;
    a.out_op = out_op;
    Down downs[3] = {{AN_OUT_ALN, n * sizeof(zsw_alignment), (void**)&a.out_aln}, {AN_OUT_INC, total * 4, (void**)&a.out_inc}, {AN_OUT_OP, total, (void**)&a.out_op}};
    if (host)
        if (zsw_error down = stage_down(ctx, ws, downs, 3)) return down;
    e = launch_annotate<true>(ctx, a, stream);
    if (e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, "annotate write", e);
    if (host) {
        ZSW_HIP(ctx, hipMemcpyAsync(out_stats, a.stats, n * 32, hipMemcpyDeviceToHost, stream));
        const size_t used[3] = {n * sizeof(zsw_alignment), total * 4, total};
        if (zsw_error down = copy_down(ctx, downs, used, 3, stream)) return down;
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
