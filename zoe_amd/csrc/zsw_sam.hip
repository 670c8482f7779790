// zsw_sam.hip — zsw_sam_batch (include/zoe_sw.h): the SAM line of every read of a batch, formatted on the device from the records
// of an alignment call (or of zsw_annotate_batch). The fields, their order and their lengths are zsw_sam.hpp (shared with
// tests/models/sam_line.cpp); this file is the wavefront behind that header's Io, the launches and the entry point.
//
// Three steps: a length launch (line_length per read, and whether the read gets the mapped shape), hipcub's exclusive sum over
// n + 1 lengths, a write launch (write_line at the place the sum gives). No atomic decides a place: the text is the same on every
// run (the one atomic counts the malformed records).
//
// One wavefront per line (SAM_G = 64 lanes), SAM_BLOCK_LINES per block, blocks striding over the batch; the record, the offsets
// and the line's start are wavefront-uniform and held in scalar registers (uni(), zsw_wave.hpp); the next line's record is
// loaded before this one is written. A line of up to SAM_LDS_LINE bytes is assembled in the wavefront's own LDS area, shifted by
// the low four bits of its address in the text, so that a 16-byte granule of the area is a 16-byte granule of the text. The flush
// writes a granule that lies wholly inside the line as one 16-byte store; the granule a line shares with its neighbour, and the
// last line's with whatever follows out_text[total], is written byte by byte with this line's bytes only: never a wide store of
// assembled and stale bytes, never a read-modify-write. Longer lines go to memory as they are formed, byte stores throughout.
// Every store, to LDS and to memory, sits behind `pos < len`: nothing outside the bytes the scan gave the line is ever written.
//
// Records, ciglets, names and offsets are caller memory: ciglets_in_range() (64-bit) comes before every ciglet load, a name or a
// read whose end lies in front of its start has length 0, and a malformed record is an unmapped line and a count.
#include <hipcub/hipcub.hpp>

#include "zsw_context.hpp"
#include "zsw_sam.hpp"
#include "zsw_wave.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::sam;
using namespace zsw::wave;

static_assert(sizeof(zsw_alignment) == sizeof(Rec), "Rec mirrors zsw_alignment");
static_assert(sizeof(zsw_alignment_stats) == 32, "zsw_alignment_stats is 32 bytes");
static_assert(ZSW_SAM_OMIT_SEQ == F_OMIT_SEQ && ZSW_STATUS_SOME == STATUS_SOME, "zsw_sam.hpp mirrors the header's values");

namespace {

enum { SM_BASES = 0, SM_OFFSETS, SM_ALN, SM_STATUS, SM_INC, SM_OP, SM_QNAMES, SM_QOFF, SM_QUALS, SM_STRAND, SM_STATS, SM_RNAME, SM_LENGTHS, SM_STARTS, SM_KIND, SM_BAD,
       SM_SCAN_TMP, SM_TEXT, SM_N };

struct SamArgs {
    const uint8_t* bases;
    const uint64_t* offsets;  // null: fixed_len
    uint32_t fixed_len;
    uint32_t n;
    const uint8_t* qnames;    // null: "*"
    const uint64_t* qoff;
    const uint8_t* quals;     // null: "*"
    const uint8_t* strand;    // null: forward
    const zsw_alignment_stats* stats;  // null: no NM
    const uint8_t* rname;     // device copy
    uint32_t rname_len, mapq;
    int flags;
    const zsw_alignment* aln;
    const uint8_t* status;
    const uint32_t* inc;
    const uint8_t* op;
    uint64_t n_ciglets;
    uint64_t* lengths;        // length launch: the bytes of every line, n + 1 entries (the last one 0)
    const uint64_t* starts;   // write launch: their exclusive sum
    uint8_t* kind;            // length launch: 1 = the mapped shape; write launch: read
    unsigned long long* n_bad;
    uint8_t* text;
};

constexpr uint32_t SAM_BLOCK = SAM_G * SAM_BLOCK_LINES;
constexpr uint32_t WAVE_LDS = SAM_LDS_LINE + 16;  // the line shifted by up to 15 bytes
static_assert(WAVE_LDS % 16 == 0, "the wavefronts' LDS areas are 16-byte granules");

// The wavefront behind the walk. tgt: byte 0 of the line, in the wavefront's LDS area or in the text; len: the bytes the scan gave
// the line — no store at or beyond it.
struct WaveIo {
    int lane;
    uint8_t* tgt;
    uint64_t len;
    const uint8_t *p_name, *p_rname, *p_seq, *p_qual;  // the read's QNAME, RNAME, the read's bases and qualities
    const uint32_t* inc;  // the record's ciglets
    const uint8_t* op;

    __device__ __forceinline__ void put8(uint64_t pos, uint64_t w, uint32_t n) const {
        if ((uint32_t)lane < n && pos + (uint32_t)lane < len) tgt[pos + (uint32_t)lane] = (uint8_t)(w >> (8 * (lane & 7)));
    }
    __device__ __forceinline__ void put_lane(uint64_t pos, uint8_t b) const {
        if (pos < len) tgt[pos] = b;
    }
    __device__ __forceinline__ void copy(uint64_t pos, const uint8_t* src, uint64_t n, bool reversed) const {
        for (uint64_t j = (uint32_t)lane; j < n; j += SAM_G)
            if (pos + j < len) tgt[pos + j] = src[reversed ? n - 1 - j : j];
    }
    __device__ __forceinline__ void name(uint64_t pos, uint64_t n) const { copy(pos, p_name, n, false); }
    __device__ __forceinline__ void rname(uint64_t pos, uint64_t n) const { copy(pos, p_rname, n, false); }
    __device__ __forceinline__ void seq(uint64_t pos, uint64_t n) const { copy(pos, p_seq, n, false); }
    __device__ __forceinline__ void qual(uint64_t pos, uint64_t n, bool reversed) const { copy(pos, p_qual, n, reversed); }

    template <bool WRITE>
    __device__ __forceinline__ uint32_t cigar_sweep(uint64_t pos, uint64_t k0, int nv, bool* bad) const {
        uint32_t i = 0, ch = 0;
        uint8_t o = 0;
        bool ok = true;
        if (lane < nv) {
            i = inc[k0 + (uint32_t)lane];
            o = op[k0 + (uint32_t)lane];
            ok = ciglet_ok(i, o);
            ch = ok ? ciglet_chars(i) : 0u;
        }
        if (__ballot(!ok)) *bad = true;
        const uint32_t x = lane_prefix_sum(ch, lane);
        if (WRITE && lane < nv && ok) put_ciglet(*this, pos + (x - ch), i, o);
        return uni((uint32_t)__shfl(x, SAM_G - 1, SAM_G));
    }
};

// WRITE = false: the length of every line (a.lengths[i]), its shape (a.kind[i]) and the count of malformed records.
// WRITE = true: the text.
template <bool WRITE>
__global__ __launch_bounds__(SAM_BLOCK) void sam_kernel(SamArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[WRITE ? SAM_BLOCK_LINES * WAVE_LDS : 16];
    const uint32_t wave = uni((uint32_t)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0) a.lengths[a.n] = 0;  // the exclusive sum's last input: its output is the total
    const uint64_t stride = (uint64_t)gridDim.x * SAM_BLOCK_LINES;
    uint64_t i = (uint64_t)blockIdx.x * SAM_BLOCK_LINES + wave;
    if (i >= a.n) return;
    zsw_alignment in = a.aln[i];
    uint8_t in_status = a.status[i];
    for (; i < a.n; i += stride) {
        const uint64_t ni = i + stride < a.n ? i + stride : i;
        const zsw_alignment next = a.aln[ni];
        const uint8_t next_status = a.status[ni];
        uint64_t off, len;
        if (a.offsets) {
            off = uni(a.offsets[i]);
            const uint64_t end = uni(a.offsets[i + 1]);
            len = end > off ? end - off : 0;
        } else {
            off = i * a.fixed_len;
            len = a.fixed_len;
        }
        uint64_t noff = 0, nlen = 0;
        if (a.qnames) {
            noff = uni(a.qoff[i]);
            const uint64_t end = uni(a.qoff[i + 1]);
            nlen = end > noff ? end - noff : 0;
        }
        const bool reversed = a.strand ? uni((uint32_t)a.strand[i]) != 0 : false;
        const Rec rec{uni(in.score), uni(in.ref_start), uni(in.ref_end), uni(in.query_start), uni(in.query_end), uni(in.ref_len), uni(in.query_len),
                      uni(in.n_ciglets), uni(in.ciglet_offset)};
        const uint8_t st = (uint8_t)uni((uint32_t)in_status);
        WaveIo io;
        io.lane = lane;
        io.tgt = nullptr;
        io.len = 0;
        io.p_name = a.qnames ? a.qnames + noff : nullptr;
        io.p_rname = a.rname;
        io.p_seq = a.bases + off;
        io.p_qual = a.quals ? a.quals + off : nullptr;
        const bool in_range = ciglets_in_range(rec, a.n_ciglets);
        io.inc = in_range ? a.inc + rec.ciglet_offset : nullptr;
        io.op = in_range ? a.op + rec.ciglet_offset : nullptr;
        const int verdict = WRITE ? (int)(uni((uint32_t)a.kind[i]) != 0) : -1;
        bool bad;
        Line L = describe(io, st, rec, a.n_ciglets, a.qnames != nullptr, nlen, len, a.quals != nullptr, (a.flags & F_OMIT_SEQ) != 0, reversed, a.rname_len,
                          a.mapq, verdict, &bad);
        if (a.stats && L.mapped) {
            const zsw_alignment_stats s = a.stats[i];
            L.has_nm = true;
            L.nm = (uint64_t)uni(s.mismatches) + (uint64_t)uni(s.ins_bases) + (uint64_t)uni(s.del_bases);
        }
        if (!WRITE) {
            const uint64_t bytes = line_length(io, L);
            if (lane == 0) {
                a.lengths[i] = bytes;
                a.kind[i] = L.mapped ? 1 : 0;
                if (bad) atomicAdd(a.n_bad, 1ull);
            }
        } else {
            const uint64_t start = uni(a.starts[i]);
            const uint64_t bytes = uni(a.starts[i + 1]) - start;
            uint8_t* dst = a.text + start;
            io.len = bytes;
            if (bytes <= SAM_LDS_LINE) {
                uint8_t* buf = lds + wave * WAVE_LDS;
                const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
                wave_sync();  // the previous line's flush has read the area
                io.tgt = buf + shift;
                write_line(io, L);
                wave_sync();
                uint8_t* g0 = dst - shift;  // 16-byte aligned; nothing in front of dst is touched
                const uint32_t span = shift + (uint32_t)bytes;
                for (uint32_t lo = 16u * (uint32_t)lane; lo < span; lo += 16u * SAM_G) {
                    if (lo >= shift && lo + 16u <= span) {
                        *reinterpret_cast<u32x4_alias*>(g0 + lo) = *reinterpret_cast<const u32x4_alias*>(buf + lo);
                    } else {  // a granule shared with a neighbour (or with what lies beyond the text): this line's bytes, one by one
                        const uint32_t b0 = lo > shift ? lo : shift, b1 = lo + 16u < span ? lo + 16u : span;
#pragma clang loop vectorize(disable) interleave(disable)  // byte stores: the loop must not become wider, unaligned ones
                        for (uint32_t b = b0; b < b1; ++b) g0[b] = buf[b];
                    }
                }
            } else {
                io.tgt = dst;
                write_line(io, L);
            }
        }
        in = next;
        in_status = next_status;
    }
}

template <bool WRITE>
hipError_t launch_sam(const zsw_context* ctx, const SamArgs& a, hipStream_t stream) {
    if (!a.n) return hipSuccess;
    const uint64_t want = ((uint64_t)a.n + SAM_BLOCK_LINES - 1) / SAM_BLOCK_LINES;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)ctx->cu_count * 8u);
    hipLaunchKernelGGL((sam_kernel<WRITE>), dim3(grid), dim3(SAM_BLOCK), 0, stream, a);
    return hipGetLastError();
}

__global__ void sam_empty_starts(uint64_t* starts) { starts[0] = 0; }

}  // namespace

extern "C" zsw_error zsw_sam_batch(zsw_context* ctx, const zsw_batch* reads, const void* fields_, int flags, const zsw_alignment* aln, const uint8_t* status,
                                   const uint32_t* inc, const uint8_t* op, uint64_t n_ciglets, uint8_t* out_text, uint64_t text_cap, uint64_t* out_n_bytes,
                                   uint64_t* out_line_offsets, uint64_t* out_n_bad, void* stream_) {
    if (!ctx) return ZSW_ERR_NOT_CONFIGURED;
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    const zsw_sam_fields* f = static_cast<const zsw_sam_fields*>(fields_);
    if (!reads || !f || !out_n_bytes || !out_n_bad) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~F_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown sam flag");
    if (f->mapq > 255) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "mapq > 255");
    if (!f->rname || f->rname_len < 1 || f->rname_len > 255) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "rname: 1..255 bytes");
    if (reads->encoding == ZSW_ENCODING_PACKED4) return fail(ctx, ZSW_ERR_UNSUPPORTED, "zsw_sam_batch takes ZSW_ENCODING_BYTES (SEQ is the reads' bytes)");
    if (reads->encoding != ZSW_ENCODING_BYTES) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.encoding");
    if (reads->mem != ZSW_MEM_HOST && reads->mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown zsw_batch.mem");
    const uint64_t n = reads->n_reads;
    if (n >= 0x7fffffffull) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "n_reads >= 2^31-1 per call");  // the scan counts n + 1 items in an int
    const bool omit_seq = (flags & F_OMIT_SEQ) != 0;
    if (n && (!aln || !status || (!reads->bases && !(omit_seq && !f->quals)))) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (n_ciglets && (!inc || !op)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null ciglet arrays");
    if (f->qnames && !f->qname_offsets) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "qnames without qname_offsets");
    if (!out_text && text_cap) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null out_text with a capacity");
    const bool host = reads->mem == ZSW_MEM_HOST;
    if (host && reads->offsets)
        for (uint64_t i = 0; i < n; ++i)
            if (reads->offsets[i + 1] < reads->offsets[i]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "offsets not monotone");
    if (host && f->qnames)
        for (uint64_t i = 0; i < n; ++i)
            if (f->qname_offsets[i + 1] < f->qname_offsets[i]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "qname_offsets not monotone");
    // bytes of the reads (and of the qualities, laid out the same way) and of the names, where the host can know them; else 1: the
    // array's first byte at least must not lie inside an output
    const size_t base_bytes = !reads->offsets ? (size_t)n * reads->fixed_len : host ? (size_t)reads->offsets[n] : 1;
    const size_t name_bytes = f->qnames ? (host ? (size_t)f->qname_offsets[n] : 1) : 0;
    {
        const void* outs[2] = {out_text, out_line_offsets};
        const size_t out_bytes[2] = {(size_t)text_cap, (size_t)(n + 1) * 8};
        const void* ins[11] = {aln, status, inc, op, reads->bases, reads->offsets, f->qnames, f->qname_offsets, f->quals, f->strand, f->stats};
        const size_t in_bytes[11] = {(size_t)n * sizeof(zsw_alignment), (size_t)n, (size_t)n_ciglets * 4, (size_t)n_ciglets, base_bytes, (size_t)(n + 1) * 8,
                                     name_bytes, (size_t)(n + 1) * 8, base_bytes, (size_t)n, (size_t)n * 32};
        for (int o = 0; o < 2; ++o)
            for (int k = 0; k < 11; ++k)
                if (overlaps(outs[o], out_bytes[o], ins[k], in_bytes[k])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "an output array overlaps an input array");
        if (overlaps(outs[0], out_bytes[0], outs[1], out_bytes[1])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "output arrays overlap");
    }
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->sam_ws;
    static_assert(SM_N <= sizeof(ctx->sam_ws) / sizeof(ctx->sam_ws[0]), "zsw_context::sam_ws holds every buffer");
    ZSW_HIP(ctx, ws[SM_LENGTHS].ensure((n + 1) * 8));
    ZSW_HIP(ctx, ws[SM_STARTS].ensure((n + 1) * 8));
    uint64_t* starts = ws[SM_STARTS].as<uint64_t>();
    if (n == 0) {
        *out_n_bytes = 0;
        *out_n_bad = 0;
        if (out_line_offsets) {
            if (host) {
                out_line_offsets[0] = 0;
            } else {
                hipLaunchKernelGGL(sam_empty_starts, dim3(1), dim3(1), 0, stream, out_line_offsets);
                ZSW_HIP(ctx, hipGetLastError());
            }
        }
        return ZSW_OK;
    }
    SamArgs a{};
    a.bases = reads->bases;
    a.offsets = reads->offsets;
    a.fixed_len = reads->fixed_len;
    a.n = (uint32_t)n;
    a.qnames = f->qnames;
    a.qoff = f->qname_offsets;
    a.quals = f->quals;
    a.strand = f->strand;
    a.stats = static_cast<const zsw_alignment_stats*>(f->stats);
    a.rname_len = f->rname_len;
    a.mapq = f->mapq;
    a.flags = flags;
    a.aln = aln;
    a.status = status;
    a.inc = inc;
    a.op = op;
    a.n_ciglets = n_ciglets;
    ZSW_HIP(ctx, ws[SM_RNAME].ensure(256));
    ZSW_HIP(ctx, ws[SM_KIND].ensure(n + 4));
    ZSW_HIP(ctx, ws[SM_BAD].ensure(16));
    ZSW_HIP(ctx, hipMemcpyAsync(ws[SM_RNAME].p, f->rname, f->rname_len, hipMemcpyHostToDevice, stream));
    ZSW_HIP(ctx, hipMemsetAsync(ws[SM_BAD].p, 0, 8, stream));
    a.rname = ws[SM_RNAME].as<uint8_t>();
    a.lengths = ws[SM_LENGTHS].as<uint64_t>();
    a.starts = starts;
    a.kind = ws[SM_KIND].as<uint8_t>();
    a.n_bad = ws[SM_BAD].as<unsigned long long>();
    if (host) {  // everything crosses once; the call returns when the text is back
        // the bases are not read under ZSW_SAM_OMIT_SEQ
        if (zsw_error up = stage_up_records(ctx, ws + SM_BASES, omit_seq ? nullptr : reads->bases, base_bytes, &a, stream)) return up;
        const Up ups[] = {
            {SM_QNAMES, f->qnames, name_bytes, (const void**)&a.qnames},
            {SM_QOFF, f->qnames ? f->qname_offsets : nullptr, (n + 1) * 8, (const void**)&a.qoff},
            {SM_QUALS, f->quals, base_bytes, (const void**)&a.quals},
            {SM_STRAND, f->strand, n, (const void**)&a.strand},
            {SM_STATS, f->stats, n * 32, (const void**)&a.stats},
        };
        if (zsw_error up = stage_up(ctx, ws, ups, 5, stream)) return up;
    }
    hipError_t e = launch_sam<false>(ctx, a, stream);
    if (e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, "sam length", e);
    size_t temp_bytes = 0;
    ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, a.lengths, starts, (int)(n + 1), stream));
    ZSW_HIP(ctx, ws[SM_SCAN_TMP].ensure(temp_bytes + 16));
    ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[SM_SCAN_TMP].p, temp_bytes, a.lengths, starts, (int)(n + 1), stream));
    uint64_t total = 0;
    unsigned long long n_bad = 0;
    ZSW_HIP(ctx, hipMemcpyAsync(&total, starts + n, 8, hipMemcpyDeviceToHost, stream));
    ZSW_HIP(ctx, hipMemcpyAsync(&n_bad, a.n_bad, 8, hipMemcpyDeviceToHost, stream));
    if (out_line_offsets) ZSW_HIP(ctx, hipMemcpyAsync(out_line_offsets, starts, (n + 1) * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    ZSW_HIP(ctx, hipStreamSynchronize(stream));  // the one synchronisation of a device call
    *out_n_bytes = total;
    *out_n_bad = n_bad;
    if (!out_text && !text_cap) return ZSW_OK;  // the sizing call
    if (total > text_cap) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "text capacity too small; required size returned");
    if (!total) return ZSW_OK;
    a.text = out_text;
    if (host) {
        ZSW_HIP(ctx, ws[SM_TEXT].ensure(total + 16));
        a.text = ws[SM_TEXT].as<uint8_t>();
    }
    e = launch_sam<true>(ctx, a, stream);
    if (e != hipSuccess) return fail(ctx, ZSW_ERR_HIP, "sam write", e);
    if (host) {
        ZSW_HIP(ctx, hipMemcpyAsync(out_text, a.text, total, hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
