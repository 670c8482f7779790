// zsw_fastq.hip — zsw_fastq_parse_batch (include/zoe_sw.h): FASTQ bytes in device memory to the arrays zsw_batch and zsw_sam_fields
// take — bases and qualities back to back with offsets, names with qname_offsets. The rules are zsw_fastq.hpp (shared with
// tests/models/fastq_parse.cpp); this file is the wavefront behind that header's Io, the launches and the entry point.
//
// Launches, all on the caller's stream, with no host step between them:
//   init      the state block (lowest failing record, min / max length)
//   count     newlines per tile of FQ_TILE bytes: 16-byte loads, the head and the tail granule peeled byte by byte
//   scan      hipcub's exclusive sum over the tile counts; its last entry is the number of newlines
//   positions the same sweep again: the position of every newline at its rank (a prefix across the lanes plus the tile's base)
//   records   one wavefront per record: parse_record -> code, name length, sequence length; an atomicMin of the lowest failing index
//   plan      one thread: delivered = min(records, lowest failing index)
//   scan x 2  exclusive sums of the name and sequence lengths of the delivered prefix -> offsets
//   gather    one wavefront per record: offsets, name, bases, qualities; nothing if a capacity is too small; min / max length
//   report    one thread: the nine words of out_info
// then one copy of the report and one synchronisation. A minimum and a maximum are the only atomics: every output is the same on
// every run. The number of newlines is not known to the host when the workspace is sized: 8 bytes per 16 bytes of text are provided
// (lines of 15 bytes and a newline on average); a denser text is found out by the report and the launches from `positions` on run
// once more with the exact size — the one case of a second synchronisation, and the context keeps the larger workspace.
#include <limits.h>

#include <hipcub/hipcub.hpp>

#include "zsw_context.hpp"
#include "zsw_fastq.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::fastq;

static_assert(ZSW_FASTQ_FINAL == F_FINAL && ZSW_FASTQ_NAME_TO_BLANK == F_NAME_TO_BLANK, "zsw_fastq.hpp mirrors the header's flags");
static_assert(ZSW_FASTQ_INFO_WORDS == INFO_WORDS && ZSW_FASTQ_INFO_MAX_LEN == INFO_MAX_LEN && ZSW_FASTQ_INFO_CONSUMED == INFO_CONSUMED,
              "zsw_fastq.hpp mirrors the header's report");
static_assert(ZSW_FASTQ_INVALID_QUALITY == INVALID_QUALITY && ZSW_FASTQ_MISSING_AT == MISSING_AT, "zsw_fastq.hpp mirrors the header's codes");

namespace {

enum { FW_TEXT = 0, FW_TILE_COUNTS, FW_TILE_BASE, FW_POS, FW_CODE, FW_NAME_LEN, FW_SEQ_LEN, FW_NAME_OFF, FW_SEQ_OFF, FW_SCAN_TMP, FW_STATE, FW_BASES, FW_QUALS,
       FW_OFFSETS, FW_QNAMES, FW_QOFF, FW_N };

// the state block: what the launches hand each other, then the report
enum { ST_FIRST_BAD = 0, ST_MIN, ST_MAX, ST_DELIVERED, ST_NEWLINES, ST_OVERFLOW, ST_WRITTEN, ST_INFO, ST_WORDS = ST_INFO + INFO_WORDS };

struct FqArgs {
    const uint8_t* text;
    uint64_t n_bytes;
    uint32_t head;            // address of text & 15
    int flags;
    uint64_t n_tiles;
    uint64_t* tile_counts;    // n_tiles + 1 (the last one 0)
    const uint64_t* tile_base;  // their exclusive sum
    uint64_t* pos;            // position of newline k, k < pos_cap
    uint64_t pos_cap;
    uint64_t rec_items;       // entries of the per-record arrays
    uint8_t* code;
    uint64_t *name_len, *seq_len;
    const uint64_t *name_off, *seq_off;  // rec_items + 1
    unsigned long long* state;
    uint8_t *out_bases, *out_quals, *out_qnames;
    uint64_t *out_offsets, *out_qname_offsets;
    uint64_t base_cap, name_cap, record_cap;
    int write;                // 0: the sizing call
};

constexpr uint32_t REC_BLOCK = FQ_G * FQ_BLOCK_RECORDS;
constexpr uint32_t TILE_BLOCK = FQ_G * FQ_TILE_WAVES;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((may_alias)) u32x4_alias;

// see zsw_annotate.hip: wavefront-uniform values loaded by vector loads, moved to scalar registers
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }

// The wavefront behind the header's walk
struct WaveIo {
    int lane;
    const uint8_t* text;
    const uint64_t* pos_in;
    uint64_t* pos_out;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const { return text[p]; }
    __device__ __forceinline__ void load16(uint64_t p, uint32_t w[4]) const {
        const u32x4 v = *reinterpret_cast<const u32x4_alias*>(text + p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    __device__ __forceinline__ uint64_t newline(uint64_t rank) const { return uni(pos_in[rank]); }
    __device__ __forceinline__ void put_position(uint64_t rank, uint64_t p) const { pos_out[rank] = p; }
    __device__ __forceinline__ bool sweep_utf8(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (uint64_t j = (uint32_t)lane; j < n; j += FQ_G) bad |= utf8_bad_at(*this, lo, n, j);
        return __ballot(bad) != 0;
    }
    __device__ __forceinline__ bool sweep_quality(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (uint64_t j = (uint32_t)lane; j < n; j += FQ_G) bad |= !quality_ok(text[lo + j]);
        return __ballot(bad) != 0;
    }
    __device__ __forceinline__ uint64_t sweep_blank(uint64_t lo, uint64_t n) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G) {
            const uint64_t j = j0 + (uint32_t)lane;
            const unsigned long long m = __ballot(j < n && is_blank(text[lo + j]));
            if (m) return j0 + (uint64_t)__builtin_ctzll(m);
        }
        return n;
    }
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 1; d < FQ_G; d <<= 1) x += __shfl_xor(x, d, FQ_G);
    return x;
}

// POSITIONS = false: tile_counts[t] = the newlines of tile t. POSITIONS = true: pos[rank] for every newline.
template <bool POSITIONS>
__global__ __launch_bounds__(TILE_BLOCK) void fq_newline_kernel(FqArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * FQ_TILE_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * FQ_TILE_WAVES;
    if (!POSITIONS && blockIdx.x == 0 && threadIdx.x == 0) a.tile_counts[a.n_tiles] = 0;  // the exclusive sum's last input: its output is the total
    WaveIo io{lane, a.text, nullptr, a.pos};
    for (uint64_t t = wave; t < a.n_tiles; t += stride) {
        uint32_t w[FQ_TILE_SWEEPS][4];
#pragma unroll
        for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) granule_words(io, a.head, a.n_bytes, (t * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane, w[s]);
        if (!POSITIONS) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) c += words_newlines(w[s]);
            c = wave_sum(c);
            if (lane == 0) a.tile_counts[t] = c;
        } else {
            uint64_t base = uni(a.tile_base[t]);
#pragma unroll
            for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) {
                const uint32_t c = words_newlines(w[s]);
                uint32_t x = c;  // inclusive prefix sum across the lanes
#pragma unroll
                for (int d = 1; d < FQ_G; d <<= 1) {
                    const uint32_t y = __shfl_up(x, d, FQ_G);
                    if (lane >= d) x += y;
                }
                if (c) put_newlines(io, w[s], a.head, (t * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane, base + (x - c), a.pos_cap);
                base += uni((uint32_t)__shfl(x, FQ_G - 1, FQ_G));
            }
        }
    }
}

__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint64_t n, int lane) {
    for (uint64_t j = (uint32_t)lane; j < n; j += FQ_G) dst[j] = src[j];
}

bool overlaps(const void* a, uint64_t na, const void* b, uint64_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

uint32_t grid_for(const zsw_context* ctx, uint64_t items, uint32_t per_block) {
    const uint64_t want = (items + per_block - 1) / per_block;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->cu_count * 8u));
}

// The newline index of a.text (text, n_bytes, head, n_tiles, tile_counts, tile_base, pos, pos_cap of `a`) on `stream`: with `count`
// the newlines per tile and their exclusive sum (a.tile_base[a.n_tiles] = how many there are), then the position of every newline
// at its rank, as far as pos_cap reaches. scan_tmp: index_scan_bytes. A caller whose workspace for the positions was an estimate
// finds tile_base[n_tiles] > pos_cap on the device, and calls once more without `count` and with the exact size.
hipError_t index_scan_bytes(const FqArgs& a, size_t* bytes, hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, a.tile_counts, const_cast<uint64_t*>(a.tile_base), (int)(a.n_tiles + 1), stream);
}
hipError_t index_launch(const zsw_context* ctx, const FqArgs& a, bool count, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (!a.n_tiles) return hipSuccess;
    const uint32_t tile_grid = grid_for(ctx, a.n_tiles, FQ_TILE_WAVES);
    if (count) {
        hipLaunchKernelGGL((fq_newline_kernel<false>), dim3(tile_grid), dim3(TILE_BLOCK), 0, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, a.tile_counts, const_cast<uint64_t*>(a.tile_base), (int)(a.n_tiles + 1), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((fq_newline_kernel<true>), dim3(tile_grid), dim3(TILE_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// zsw_samtext.hip includes this file for everything above (the wavefront behind the header's Io, the newline index) and defines
// ZSW_FASTQ_INDEX_ONLY to leave out what follows: the FASTQ records and the entry point.
#ifndef ZSW_FASTQ_INDEX_ONLY

__global__ void fq_init_kernel(unsigned long long* state) {
    for (int k = 0; k < ST_WORDS; ++k) state[k] = 0;
    state[ST_FIRST_BAD] = ~0ull;
    state[ST_MIN] = ~0ull;
}

// what every later launch first asks: how many newlines, how many records; false: the positions did not fit, nothing is done
__device__ __forceinline__ bool fq_text(const FqArgs& a, Text* t, uint64_t* n_rec) {
    t->n_bytes = a.n_bytes;
    t->n_newlines = a.n_tiles ? uni(a.tile_base[a.n_tiles]) : 0;
    t->flags = a.flags;
    if (t->n_newlines > a.pos_cap) return false;
    const bool last_nl = a.n_bytes ? uni((uint32_t)a.text[a.n_bytes - 1]) == '\n' : true;
    *n_rec = n_records(*t, last_nl);
    return *n_rec <= a.rec_items;  // holds by the sizes the entry point gives the arrays
}

__global__ __launch_bounds__(REC_BLOCK) void fq_record_kernel(FqArgs a) {
    const int lane = threadIdx.x & 63;
    Text t;
    uint64_t n_rec;
    if (!fq_text(a, &t, &n_rec)) return;
    WaveIo io{lane, a.text, a.pos, nullptr};
    const uint64_t stride = (uint64_t)gridDim.x * FQ_BLOCK_RECORDS;
    uint64_t first_bad = ~0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * FQ_BLOCK_RECORDS + uni((uint32_t)(threadIdx.x >> 6)); r < n_rec; r += stride) {
        const Record R = parse_record(io, t, r);
        if (lane == 0) {
            a.code[r] = (uint8_t)R.code;
            a.name_len[r] = R.name_len;
            a.seq_len[r] = R.seq_len;
        }
        if (R.code && r < first_bad) first_bad = r;
    }
    if (lane == 0 && first_bad != ~0ull) atomicMin(&a.state[ST_FIRST_BAD], (unsigned long long)first_bad);
}

__global__ void fq_plan_kernel(FqArgs a) {
    Text t;
    uint64_t n_rec;
    a.state[ST_NEWLINES] = a.n_tiles ? a.tile_base[a.n_tiles] : 0;
    if (!fq_text(a, &t, &n_rec)) {
        a.state[ST_OVERFLOW] = 1;
        a.state[ST_DELIVERED] = 0;
        return;
    }
    const uint64_t fb = a.state[ST_FIRST_BAD];
    a.state[ST_DELIVERED] = fb < n_rec ? fb : n_rec;
}

// the lengths of the delivered prefix, 0 behind it: what the two offset scans sum
struct DeliveredLength {
    const uint64_t* len;
    const unsigned long long* delivered;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i < *delivered ? len[i] : 0; }
};
typedef hipcub::TransformInputIterator<uint64_t, DeliveredLength, hipcub::CountingInputIterator<uint64_t>> LengthIter;

__global__ __launch_bounds__(REC_BLOCK) void fq_gather_kernel(FqArgs a) {
    const int lane = threadIdx.x & 63;
    if (a.state[ST_OVERFLOW]) return;
    Text t;
    uint64_t n_rec;
    if (!fq_text(a, &t, &n_rec)) return;
    const uint64_t n = uni((uint64_t)a.state[ST_DELIVERED]);
    const uint64_t bases = uni(a.seq_off[n]), names = uni(a.name_off[n]);
    const bool want_names = a.out_qnames != nullptr;
    const bool write = a.write && n <= a.record_cap && bases <= a.base_cap && (!want_names || names <= a.name_cap);
    WaveIo io{lane, a.text, a.pos, nullptr};
    const uint32_t wave = uni((uint32_t)(threadIdx.x >> 6));
    if (write && blockIdx.x == 0 && wave == 0 && lane == 0) {
        a.out_offsets[n] = bases;
        if (want_names) a.out_qname_offsets[n] = names;
        a.state[ST_WRITTEN] = 1;
    }
    const uint64_t stride = (uint64_t)gridDim.x * FQ_BLOCK_RECORDS;
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FQ_BLOCK_RECORDS + wave; r < n; r += stride) {
        const uint64_t s0 = uni(a.seq_off[r]), s_len = uni(a.seq_off[r + 1]) - s0;
        lo = s_len < lo ? s_len : lo;
        hi = s_len > hi ? s_len : hi;
        if (!write) continue;
        const Record R = locate_record(io, t, r);
        // a good record: name, bases and qualities lie inside its lines; the lengths are asked once more, in 64 bits, before the loads
        if (R.seq_lo + s_len > t.n_bytes || R.qual_lo + s_len > t.n_bytes || s0 + s_len > a.base_cap) continue;
        wave_copy(a.out_bases + s0, a.text + R.seq_lo, s_len, lane);
        if (a.out_quals) wave_copy(a.out_quals + s0, a.text + R.qual_lo, s_len, lane);
        if (lane == 0) a.out_offsets[r] = s0;
        if (want_names) {
            const uint64_t n0 = uni(a.name_off[r]), n_len = uni(a.name_off[r + 1]) - n0;
            if (R.name_lo + n_len > t.n_bytes || n0 + n_len > a.name_cap) continue;
            wave_copy(a.out_qnames + n0, a.text + R.name_lo, n_len, lane);
            if (lane == 0) a.out_qname_offsets[r] = n0;
        }
    }
    if (lane == 0 && hi) {
        atomicMin(&a.state[ST_MIN], (unsigned long long)lo);
        atomicMax(&a.state[ST_MAX], (unsigned long long)hi);
    }
}

__global__ void fq_report_kernel(FqArgs a) {
    unsigned long long* info = a.state + ST_INFO;
    Text t;
    uint64_t n_rec;
    if (a.state[ST_OVERFLOW] || !fq_text(a, &t, &n_rec)) return;
    WaveIo io{0, a.text, a.pos, nullptr};
    const uint64_t n = a.state[ST_DELIVERED];
    info[INFO_RECORDS] = n;
    info[INFO_BASES] = a.seq_off[n];
    info[INFO_NAME_BYTES] = a.name_off[n];
    info[INFO_CONSUMED] = line_start(io, t, 4u * n);
    if (n < n_rec) {
        info[INFO_ERROR] = a.code[n];
        info[INFO_ERROR_RECORD] = n;
        info[INFO_ERROR_OFFSET] = line_start(io, t, 4u * n);
    }
    info[INFO_MIN_LEN] = n ? a.state[ST_MIN] : 0;
    info[INFO_MAX_LEN] = a.state[ST_MAX];
}

#endif  // ZSW_FASTQ_INDEX_ONLY

}  // namespace

#ifndef ZSW_FASTQ_INDEX_ONLY
extern "C" zsw_error zsw_fastq_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags, uint8_t* out_bases, uint8_t* out_quals,
                                           uint64_t base_cap, uint64_t* out_offsets, uint8_t* out_qnames, uint64_t name_cap, uint64_t* out_qname_offsets,
                                           uint64_t record_cap, uint64_t* out_info, void* stream_) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!out_info || (n_bytes && !text)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~F_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown fastq flag");
    if (mem != ZSW_MEM_HOST && mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown mem");
    const bool sizing = !out_bases && !out_quals && !out_offsets && !out_qnames && !out_qname_offsets && !base_cap && !name_cap && !record_cap;
    if (!sizing && (!out_bases || !out_offsets)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null out_bases / out_offsets outside the sizing call");
    if ((out_qnames == nullptr) != (out_qname_offsets == nullptr)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "out_qnames and out_qname_offsets go together");
    if (n_bytes > (1ull << 36)) return fail(ctx, ZSW_ERR_UNSUPPORTED, "more than 2^36 bytes per call: parse the file in chunks");
    if (record_cap >= (1ull << 60)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "record_cap");
    const bool want_names = out_qnames != nullptr;
    if (!want_names) name_cap = 0;
    {
        const void* p[6] = {text, out_bases, out_quals, out_offsets, out_qnames, out_qname_offsets};
        const uint64_t b[6] = {n_bytes, base_cap, base_cap, (record_cap + 1) * 8, name_cap, (record_cap + 1) * 8};
        for (int i = 0; i < 6; ++i)
            for (int k = i + 1; k < 6; ++k)
                if (overlaps(p[i], b[i], p[k], b[k])) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, i ? "output arrays overlap" : "an output array overlaps the text");
    }
    const bool host = mem == ZSW_MEM_HOST;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->fq_ws;
    static_assert(FW_N <= sizeof(ctx->fq_ws) / sizeof(ctx->fq_ws[0]), "zsw_context::fq_ws holds every buffer");
    FqArgs a{};
    a.text = text;
    a.n_bytes = n_bytes;
    a.flags = flags;
    a.out_bases = out_bases;
    a.out_quals = out_quals;
    a.out_qnames = out_qnames;
    a.out_offsets = out_offsets;
    a.out_qname_offsets = out_qname_offsets;
    a.base_cap = base_cap;
    a.name_cap = name_cap;
    a.record_cap = record_cap;
    a.write = sizing ? 0 : 1;
    if (host) {  // the text crosses once; the outputs are formed in workspace no larger than the bounds that always suffice
        ZSW_HIP(ctx, ws[FW_TEXT].ensure(n_bytes + 16));
        if (n_bytes) ZSW_HIP(ctx, hipMemcpyAsync(ws[FW_TEXT].p, text, n_bytes, hipMemcpyHostToDevice, stream));
        a.text = ws[FW_TEXT].as<uint8_t>();
        if (!sizing) {
            a.base_cap = std::min<uint64_t>(base_cap, n_bytes / 2);
            a.name_cap = std::min<uint64_t>(name_cap, n_bytes);
            a.record_cap = std::min<uint64_t>(record_cap, n_bytes / 8 + 1);
            ZSW_HIP(ctx, ws[FW_BASES].ensure(a.base_cap + 16));
            ZSW_HIP(ctx, ws[FW_OFFSETS].ensure((a.record_cap + 1) * 8));
            a.out_bases = ws[FW_BASES].as<uint8_t>();
            a.out_offsets = ws[FW_OFFSETS].as<uint64_t>();
            if (out_quals) {
                ZSW_HIP(ctx, ws[FW_QUALS].ensure(a.base_cap + 16));
                a.out_quals = ws[FW_QUALS].as<uint8_t>();
            }
            if (want_names) {
                ZSW_HIP(ctx, ws[FW_QNAMES].ensure(a.name_cap + 16));
                ZSW_HIP(ctx, ws[FW_QOFF].ensure((a.record_cap + 1) * 8));
                a.out_qnames = ws[FW_QNAMES].as<uint8_t>();
                a.out_qname_offsets = ws[FW_QOFF].as<uint64_t>();
            }
        }
    }
    a.head = (uint32_t)(reinterpret_cast<uintptr_t>(a.text) & 15u);
    a.n_tiles = tiles_of(a.head, n_bytes);
    ZSW_HIP(ctx, ws[FW_TILE_COUNTS].ensure((a.n_tiles + 1) * 8));
    ZSW_HIP(ctx, ws[FW_TILE_BASE].ensure((a.n_tiles + 1) * 8));
    ZSW_HIP(ctx, ws[FW_STATE].ensure(ST_WORDS * 8));
    a.tile_counts = ws[FW_TILE_COUNTS].as<uint64_t>();
    a.tile_base = ws[FW_TILE_BASE].as<uint64_t>();
    a.state = ws[FW_STATE].as<unsigned long long>();
    unsigned long long state[ST_WORDS] = {};
    uint64_t want_pos = std::max<uint64_t>(n_bytes / 16 + 64, ws[FW_POS].cap / 8);
    for (int round = 0; round < 2; ++round) {
        // the per-record arrays hold ceil((newlines + 1) / 4) records: as many as want_pos newlines can make
        ZSW_HIP(ctx, ws[FW_POS].ensure(want_pos * 8));
        a.pos_cap = want_pos;
        a.rec_items = want_pos / 4 + 1;
        // hipcub counts its items in an int: the first round's estimate always fits (n_bytes <= 2^36), an exact count of newlines may not
        if (a.rec_items + 1 > (uint64_t)INT_MAX) return fail(ctx, ZSW_ERR_UNSUPPORTED, "fastq: more than 2^33 newlines per call: parse the file in chunks");
        ZSW_HIP(ctx, ws[FW_CODE].ensure(a.rec_items));
        ZSW_HIP(ctx, ws[FW_NAME_LEN].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[FW_SEQ_LEN].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[FW_NAME_OFF].ensure((a.rec_items + 1) * 8));
        ZSW_HIP(ctx, ws[FW_SEQ_OFF].ensure((a.rec_items + 1) * 8));
        a.pos = ws[FW_POS].as<uint64_t>();
        a.code = ws[FW_CODE].as<uint8_t>();
        a.name_len = ws[FW_NAME_LEN].as<uint64_t>();
        a.seq_len = ws[FW_SEQ_LEN].as<uint64_t>();
        uint64_t* name_off = ws[FW_NAME_OFF].as<uint64_t>();
        uint64_t* seq_off = ws[FW_SEQ_OFF].as<uint64_t>();
        a.name_off = name_off;
        a.seq_off = seq_off;
        const int scan_items = (int)(a.rec_items + 1);
        const LengthIter name_in(hipcub::CountingInputIterator<uint64_t>(0), DeliveredLength{a.name_len, a.state + ST_DELIVERED});
        const LengthIter seq_in(hipcub::CountingInputIterator<uint64_t>(0), DeliveredLength{a.seq_len, a.state + ST_DELIVERED});
        size_t tmp_tiles = 0, tmp_names = 0, tmp_seqs = 0;
        ZSW_HIP(ctx, index_scan_bytes(a, &tmp_tiles, stream));
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_names, name_in, name_off, scan_items, stream));
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_seqs, seq_in, seq_off, scan_items, stream));
        ZSW_HIP(ctx, ws[FW_SCAN_TMP].ensure(std::max(tmp_tiles, std::max(tmp_names, tmp_seqs)) + 16));

        hipLaunchKernelGGL(fq_init_kernel, dim3(1), dim3(1), 0, stream, a.state);
        if (a.n_tiles) {
            ZSW_HIP(ctx, index_launch(ctx, a, round == 0, ws[FW_SCAN_TMP].p, tmp_tiles, stream));
            hipLaunchKernelGGL(fq_record_kernel, dim3(grid_for(ctx, a.rec_items, FQ_BLOCK_RECORDS)), dim3(REC_BLOCK), 0, stream, a);
        }
        hipLaunchKernelGGL(fq_plan_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[FW_SCAN_TMP].p, tmp_names, name_in, name_off, scan_items, stream));
        ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(ws[FW_SCAN_TMP].p, tmp_seqs, seq_in, seq_off, scan_items, stream));
        hipLaunchKernelGGL(fq_gather_kernel, dim3(grid_for(ctx, a.rec_items, FQ_BLOCK_RECORDS)), dim3(REC_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(fq_report_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, hipMemcpyAsync(state, a.state, sizeof(state), hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipStreamSynchronize(stream));  // the one synchronisation of a device call
        if (!state[ST_OVERFLOW]) break;
        if (round == 1) return fail(ctx, ZSW_ERR_HIP, "fastq: the newline positions did not fit twice");
        want_pos = state[ST_NEWLINES] + 64;  // a text denser than a newline per 16 bytes: once more, from the positions on
    }
    for (int k = 0; k < INFO_WORDS; ++k) out_info[k] = state[ST_INFO + k];
    if (sizing) return ZSW_OK;
    if (!state[ST_WRITTEN]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a capacity is too small; required sizes returned in out_info");
    if (host) {
        const uint64_t n = out_info[INFO_RECORDS];
        if (out_info[INFO_BASES]) ZSW_HIP(ctx, hipMemcpyAsync(out_bases, a.out_bases, out_info[INFO_BASES], hipMemcpyDeviceToHost, stream));
        if (out_quals && out_info[INFO_BASES]) ZSW_HIP(ctx, hipMemcpyAsync(out_quals, a.out_quals, out_info[INFO_BASES], hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipMemcpyAsync(out_offsets, a.out_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
        if (want_names) {
            if (out_info[INFO_NAME_BYTES]) ZSW_HIP(ctx, hipMemcpyAsync(out_qnames, a.out_qnames, out_info[INFO_NAME_BYTES], hipMemcpyDeviceToHost, stream));
            ZSW_HIP(ctx, hipMemcpyAsync(out_qname_offsets, a.out_qname_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
        }
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
#endif  // ZSW_FASTQ_INDEX_ONLY
