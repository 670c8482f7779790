// zsw_fasta.hip — zsw_fasta_parse_batch (include/zoe_sw.h): FASTA bytes in device memory to the arrays zsw_batch, zsw_sam_fields and
// zsw_set_reference take — sequences back to back with offsets, names with name offsets. The rules are zsw_fasta.hpp (shared with
// tests/models/fasta_parse.cpp); the index of the '>' bytes is zsw_text.hip's newline index instantiated for '>'; the state block,
// the sums and the rounds are zsw_text_dev.hpp. This file is the wavefronts behind the header's Io, their launches and the entry point.
//
// Launches, all on the caller's stream, with no host step between them:
//   init      the state block (lowest failing record, min / max length)
//   index     zsw_text.hip: '>' per tile, their exclusive sum, the position of every '>' at its rank
//   records   one wavefront per record: parse_record -> code, name length, where the body starts; one wavefront more for the start
//             of the file; an atomicMin of the lowest failing index. Its work follows header lengths, not sequence lengths
//   plan      one thread: delivered = min(records, lowest failing index), and the cut: the '>' of the first record not delivered
//   scan      exclusive sum of the name lengths of the delivered prefix
//   count     one wavefront per tile of the text: the bytes that stay (in a body, in front of the cut, no line break)
//   scan      their exclusive sum over the tiles; its last entry is the number of bases
//   write     the same sweep again: every kept byte to its rank (a prefix across the lanes plus the tile's base); the lane that holds
//             '>' r writes the number of bases in front of it — offset r. Nothing to the caller's arrays if a capacity is too small
//   gather    one wavefront per record: offsets to the caller, the name, min / max length
//   report    one thread: the nine words of out_info
// then one copy of the report and one synchronisation. No launch walks a sequence record by record: a text of ten million short
// records and one record of the same size take the same sweeps over the same tiles. A minimum and a maximum are the only atomics:
// every output is the same on every run. The number of '>' is not known to the host when the workspace is sized: 8 bytes per 64
// bytes of text are provided; a denser text is found out by the report and the launches from `positions` on run once more with the
// exact size — the one case of a second synchronisation, and the context keeps the larger workspace.
#include "zsw_text_dev.hpp"

#include "zsw_fasta.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::fasta;

static_assert(ZSW_FASTA_FINAL == F_FINAL && ZSW_FASTA_NAME_TO_BLANK == F_NAME_TO_BLANK && ZSW_FASTA_CONTINUED == F_CONTINUED, "zsw_fasta.hpp mirrors the header's flags");
static_assert(ZSW_FASTA_INFO_WORDS == INFO_WORDS && ZSW_FASTA_INFO_MAX_LEN == INFO_MAX_LEN && ZSW_FASTA_INFO_CONSUMED == INFO_CONSUMED,
              "zsw_fasta.hpp mirrors the header's report");
static_assert(ZSW_FASTA_NO_DATA == NO_DATA && ZSW_FASTA_GT_IN_SEQUENCE == GT_IN_SEQUENCE, "zsw_fasta.hpp mirrors the header's codes");

namespace {

enum { AW_CODE = 0, AW_NAME_LEN, AW_BODY_LO, AW_NAME_OFF, AW_SEQ_OFF, AW_KEPT, AW_KEPT_BASE, AW_SCAN_TMP, AW_STATE, AW_BASES, AW_OFFSETS, AW_NAMES, AW_NOFF, AW_N };

// the state block behind the report words: the start of the file, the cut, a CONTINUED text that does not start with '>'
enum { ST_START_CODE = ST_INFO + INFO_WORDS, ST_START_OFFSET, ST_START_CONSUMED, ST_CUT, ST_BAD_START, ST_WORDS };

struct FaArgs {
    IndexArgs ix;             // the '>' index: text, n_bytes, head, tiles, pos, pos_cap
    int flags;
    uint64_t rec_items;       // entries of the per-record arrays
    uint8_t* code;
    uint64_t *name_len, *body_lo;
    const uint64_t* name_off;  // rec_items + 1
    uint64_t* seq_off;         // rec_items + 1: bases in front of '>' r
    uint64_t* kept;            // n_tiles + 1 (the last one 0)
    const uint64_t* kept_base;  // their exclusive sum
    unsigned long long* state;
    uint8_t *out_bases, *out_names;
    uint64_t *out_offsets, *out_name_offsets;
    uint64_t base_cap, name_cap, record_cap;
    int write;                // 0: the sizing call
};

constexpr uint32_t REC_BLOCK = FQ_G * FA_BLOCK_RECORDS;
constexpr uint32_t TILE_BLOCK = FQ_G * FQ_TILE_WAVES;

// The wavefront behind the header's walk over one record
struct WaveIo : WaveSweeps<WaveIo> {
    int lane;
    const uint8_t* text;
    const uint64_t* pos_in;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const { return text[p]; }
    __device__ __forceinline__ uint64_t sweep_class(uint64_t lo, uint64_t n, int cls) const {
        return sweep_first(lo, n, [cls](uint8_t c) { return in_class(c, cls); });
    }
    __device__ __forceinline__ uint64_t sweep_class_last(uint64_t lo, uint64_t n, int cls) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G) {
            const uint64_t j = j0 + (uint32_t)lane;
            const unsigned long long m = __ballot(j < n && in_class(text[lo + (n - 1u - (j < n ? j : 0u))], cls));
            if (m) return n - 1u - (j0 + (uint64_t)__builtin_ctzll(m));
        }
        return n;
    }
};

// The lane behind granule_words and granule_bases in the two sweeps of the sequence pass
struct TileIo {
    const uint8_t* text;
    const uint64_t* body;
    uint8_t* bases;      // null: not written (a capacity is too small, or the sizing call)
    uint64_t* off;
    uint64_t base_cap, off_items;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const { return text[p]; }
    __device__ __forceinline__ void load16(uint64_t p, uint32_t w[4]) const {
        const u32x4 v = *reinterpret_cast<const u32x4_alias*>(text + p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    __device__ __forceinline__ uint64_t body_lo(uint64_t r) const { return body[r]; }
    __device__ __forceinline__ void put_base(uint64_t rank, uint8_t c) const {
        if (bases && rank < base_cap) bases[rank] = c;
    }
    __device__ __forceinline__ void put_offset(uint64_t r, uint64_t kept) const {
        if (r < off_items) off[r] = kept;
    }
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 1; d < FQ_G; d <<= 1) x += __shfl_xor(x, d, FQ_G);
    return x;
}

__device__ __forceinline__ bool fa_text(const FaArgs& a, Text* t, uint64_t* n_rec) { return text_of<n_records>(a.ix, a.flags, a.rec_items, t, n_rec); }

__global__ __launch_bounds__(REC_BLOCK) void fa_record_kernel(FaArgs a) {
    const int lane = threadIdx.x & 63;
    Text t;
    uint64_t n_rec;
    if (!fa_text(a, &t, &n_rec)) return;
    WaveIo io{{}, lane, a.ix.text, a.ix.pos};
    const uint32_t wave = uni((uint32_t)(threadIdx.x >> 6));
    const uint64_t stride = (uint64_t)gridDim.x * FA_BLOCK_RECORDS;
    uint64_t first_bad = ~0ull;
    if (blockIdx.x == 0 && wave == 0 && !(a.flags & F_CONTINUED)) {  // the start of the file
        const Start s = check_start(io, t);
        if (lane == 0) {
            a.state[ST_START_CODE] = s.code;
            a.state[ST_START_OFFSET] = s.offset;
            a.state[ST_START_CONSUMED] = s.consumed;
        }
        if (s.code) first_bad = 0;
    }
    for (uint64_t r = (uint64_t)blockIdx.x * FA_BLOCK_RECORDS + wave; r < n_rec; r += stride) {
        const Record R = parse_record(io, t, r);
        if (lane == 0) {
            a.code[r] = (uint8_t)R.code;
            a.name_len[r] = R.name_len;
            a.body_lo[r] = R.body_lo;
        }
        if (R.code && r < first_bad) first_bad = r;
    }
    if (lane == 0 && first_bad != ~0ull) atomicMin(&a.state[ST_FIRST_BAD], (unsigned long long)first_bad);
}

// one thread: delivered = min(records, lowest failing index); the cut
__global__ void fa_plan_kernel(FaArgs a) {
    Text t;
    uint64_t n;
    a.state[ST_NEWLINES] = a.ix.n_tiles ? a.ix.tile_base[a.ix.n_tiles] : 0;
    a.state[ST_DELIVERED] = 0;
    if (!fa_text(a, &t, &n)) {
        a.state[ST_OVERFLOW] = 1;
        return;
    }
    if ((a.flags & F_CONTINUED) && (!a.ix.n_bytes || a.ix.text[0] != '>')) {
        a.state[ST_BAD_START] = 1;
        return;
    }
    WaveIo io{{}, 0, a.ix.text, a.ix.pos};
    const uint64_t fb = a.state[ST_FIRST_BAD];
    const uint64_t d = fb < n ? fb : n;
    a.state[ST_DELIVERED] = d;
    a.state[ST_CUT] = gt_at(io, t, d);
}

// the lengths of the delivered prefix, 0 behind it: what the name offset scan sums
struct DeliveredLength {
    const uint64_t* len;
    const unsigned long long* delivered;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i < *delivered ? len[i] : 0; }
};

// do the caller's arrays hold what the call delivers? (asked behind the second scan: the number of bases is kept_base[n_tiles])
__device__ __forceinline__ bool fa_fits(const FaArgs& a, uint64_t n, uint64_t bases, uint64_t names) {
    return a.write && n <= a.record_cap && bases <= a.base_cap && (!a.out_names || names <= a.name_cap);
}

// WRITE = false: kept[t] = the bytes of tile t that stay. WRITE = true: every one of them at its rank, seq_off[r] for every '>'.
template <bool WRITE>
__global__ __launch_bounds__(TILE_BLOCK) void fa_sequence_kernel(FaArgs a) {
    const int lane = threadIdx.x & 63;
    if (!WRITE && blockIdx.x == 0 && threadIdx.x == 0) a.kept[a.ix.n_tiles] = 0;  // the exclusive sum's last input: its output is the total
    if (a.state[ST_OVERFLOW] || a.state[ST_BAD_START]) return;
    Text t;
    uint64_t n_rec;
    if (!fa_text(a, &t, &n_rec)) return;
    const uint64_t n = uni((uint64_t)a.state[ST_DELIVERED]), cut = uni((uint64_t)a.state[ST_CUT]);
    TileIo io{a.ix.text, a.body_lo, nullptr, a.seq_off, a.base_cap, a.rec_items + 1};
    if (WRITE && fa_fits(a, n, uni(a.kept_base[a.ix.n_tiles]), uni(a.name_off[n]))) io.bases = a.out_bases;
    const uint64_t wave = (uint64_t)blockIdx.x * FQ_TILE_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * FQ_TILE_WAVES;
    for (uint64_t tl = wave; tl < a.ix.n_tiles; tl += stride) {
        uint32_t w[FQ_TILE_SWEEPS][4];
#pragma unroll
        for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) granule_words(io, a.ix.head, a.ix.n_bytes, (tl * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane, w[s]);
        uint64_t gts = uni(a.ix.tile_base[tl]);                 // '>' in front of the sweep
        uint64_t rank = WRITE ? uni(a.kept_base[tl]) : 0;       // kept bytes in front of the sweep
        uint32_t total = 0;
#pragma unroll
        for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) {
            const uint64_t g = (tl * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane;
            const uint32_t c = words_newlines<'>'>(w[s]);
            const uint32_t x = lane_prefix_sum(c, lane);
            if (!WRITE) {
                total += granule_bases<false>(io, w[s], a.ix.head, a.ix.n_bytes, g, gts + (x - c), n_rec, cut, 0);
            } else {
                const uint32_t k = granule_bases<false>(io, w[s], a.ix.head, a.ix.n_bytes, g, gts + (x - c), n_rec, cut, 0);
                const uint32_t y = lane_prefix_sum(k, lane);
                if (k || c) granule_bases<true>(io, w[s], a.ix.head, a.ix.n_bytes, g, gts + (x - c), n_rec, cut, rank + (y - k));
                rank += uni((uint32_t)__shfl(y, FQ_G - 1, FQ_G));
            }
            gts += uni((uint32_t)__shfl(x, FQ_G - 1, FQ_G));
        }
        if (!WRITE) {
            total = wave_sum(total);
            if (lane == 0) a.kept[tl] = total;
        }
    }
}

__global__ __launch_bounds__(REC_BLOCK) void fa_gather_kernel(FaArgs a) {
    const int lane = threadIdx.x & 63;
    if (a.state[ST_OVERFLOW] || a.state[ST_BAD_START]) return;
    Text t;
    uint64_t n_rec;
    if (!fa_text(a, &t, &n_rec)) return;
    const uint64_t n = uni((uint64_t)a.state[ST_DELIVERED]);
    const uint64_t bases = a.ix.n_tiles ? uni(a.kept_base[a.ix.n_tiles]) : 0, names = uni(a.name_off[n]);
    const bool want_names = a.out_names != nullptr;
    const bool write = fa_fits(a, n, bases, names);
    WaveIo io{{}, lane, a.ix.text, a.ix.pos};
    const uint32_t wave = uni((uint32_t)(threadIdx.x >> 6));
    if (write && blockIdx.x == 0 && wave == 0 && lane == 0) {
        a.out_offsets[n] = bases;
        if (want_names) a.out_name_offsets[n] = names;
        a.state[ST_WRITTEN] = 1;
    }
    const uint64_t stride = (uint64_t)gridDim.x * FA_BLOCK_RECORDS;
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * FA_BLOCK_RECORDS + wave; r < n; r += stride) {
        const uint64_t s0 = uni(a.seq_off[r]), s1 = r + 1u < n ? uni(a.seq_off[r + 1]) : bases;
        const uint64_t s_len = s1 - s0;
        lo = s_len < lo ? s_len : lo;
        hi = s_len > hi ? s_len : hi;
        if (!write) continue;
        if (lane == 0) a.out_offsets[r] = s0;
        if (want_names) {
            const uint64_t n0 = uni(a.name_off[r]), n_len = uni(a.name_off[r + 1]) - n0;
            const uint64_t n_lo = name_start(io, t, r);
            // a good record: the name lies inside its region; the lengths are asked once more, in 64 bits, before the loads
            if (n_lo + n_len > t.n_bytes || n0 + n_len > a.name_cap) continue;
            wave_copy(a.out_names + n0, a.ix.text + n_lo, n_len, lane);
            if (lane == 0) a.out_name_offsets[r] = n0;
        }
    }
    if (lane == 0 && hi) {
        atomicMin(&a.state[ST_MIN], (unsigned long long)lo);
        atomicMax(&a.state[ST_MAX], (unsigned long long)hi);
    }
}

__global__ void fa_report_kernel(FaArgs a) {
    unsigned long long* info = a.state + ST_INFO;
    Text t;
    uint64_t n_rec;
    if (a.state[ST_OVERFLOW] || a.state[ST_BAD_START] || !fa_text(a, &t, &n_rec)) return;
    const uint64_t n = a.state[ST_DELIVERED];
    const uint64_t start_code = a.state[ST_START_CODE];
    info[INFO_RECORDS] = n;
    info[INFO_BASES] = a.ix.n_tiles ? a.kept_base[a.ix.n_tiles] : 0;
    info[INFO_NAME_BYTES] = a.name_off[n];
    info[INFO_CONSUMED] = start_code ? 0 : t.n_newlines ? a.state[ST_CUT] : a.state[ST_START_CONSUMED];
    if (start_code) {
        info[INFO_ERROR] = start_code;
        info[INFO_ERROR_OFFSET] = a.state[ST_START_OFFSET];
    } else if (n < n_rec) {
        info[INFO_ERROR] = a.code[n];
        info[INFO_ERROR_RECORD] = n;
        info[INFO_ERROR_OFFSET] = a.state[ST_CUT];
    }
    info[INFO_MIN_LEN] = n ? a.state[ST_MIN] : 0;
    info[INFO_MAX_LEN] = a.state[ST_MAX];
}

}  // namespace

extern "C" zsw_error zsw_fasta_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags, uint8_t* out_bases, uint64_t base_cap,
                                           uint64_t* out_offsets, uint8_t* out_names, uint64_t name_cap, uint64_t* out_name_offsets, uint64_t record_cap,
                                           uint64_t* out_info, void* stream_) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!out_info || (n_bytes && !text)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~F_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown fasta flag");
    if (mem != ZSW_MEM_HOST && mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown mem");
    const bool sizing = !out_bases && !out_offsets && !out_names && !out_name_offsets && !base_cap && !name_cap && !record_cap;
    if (!sizing && (!out_bases || !out_offsets)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null out_bases / out_offsets outside the sizing call");
    if ((out_names == nullptr) != (out_name_offsets == nullptr)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "out_names and out_name_offsets go together");
    if (n_bytes > (1ull << 36)) return fail(ctx, ZSW_ERR_UNSUPPORTED, "more than 2^36 bytes per call: parse the file in chunks");
    if (record_cap >= (1ull << 60)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "record_cap");
    const bool want_names = out_names != nullptr;
    if (!want_names) name_cap = 0;
    const Span spans[5] = {{text, n_bytes}, {out_bases, base_cap}, {out_offsets, (record_cap + 1) * 8}, {out_names, name_cap}, {out_name_offsets, (record_cap + 1) * 8}};
    if (const int i = first_overlap(spans, 5); i >= 0) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, i ? "output arrays overlap" : "an output array overlaps the text");
    const bool host = mem == ZSW_MEM_HOST;
    const char* bad_start = "ZSW_FASTA_CONTINUED: the text does not start with '>'";
    if ((flags & F_CONTINUED) && (!n_bytes || (host && text[0] != '>'))) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, bad_start);
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->fa_ws;
    static_assert(AW_N <= sizeof(ctx->fa_ws) / sizeof(ctx->fa_ws[0]), "zsw_context::fa_ws holds every buffer");
    FaArgs a{};
    a.flags = flags;
    a.out_bases = out_bases;
    a.out_names = out_names;
    a.out_offsets = out_offsets;
    a.out_name_offsets = out_name_offsets;
    a.base_cap = base_cap;
    a.name_cap = name_cap;
    a.record_cap = record_cap;
    a.write = sizing ? 0 : 1;
    if (zsw_error e = index_prepare(ctx, &a.ix, text, n_bytes, host, stream)) return e;
    const bool staged = host && !sizing;  // the outputs are formed in workspace no larger than the bounds that always suffice
    if (staged) {
        a.base_cap = std::min<uint64_t>(base_cap, n_bytes);
        a.name_cap = std::min<uint64_t>(name_cap, n_bytes);
        a.record_cap = std::min<uint64_t>(record_cap, n_bytes / 4 + 1);
    }
    Down downs[4] = {{AW_BASES, a.base_cap, (void**)&a.out_bases}, {AW_OFFSETS, (a.record_cap + 1) * 8, (void**)&a.out_offsets}, {AW_NAMES, a.name_cap, (void**)&a.out_names},
                     {AW_NOFF, (a.record_cap + 1) * 8, (void**)&a.out_name_offsets}};
    if (staged)
        if (zsw_error e = stage_down(ctx, ws, downs, 4)) return e;
    ZSW_HIP(ctx, ws[AW_STATE].ensure(ST_WORDS * 8));
    ZSW_HIP(ctx, ws[AW_KEPT].ensure((a.ix.n_tiles + 1) * 8));
    ZSW_HIP(ctx, ws[AW_KEPT_BASE].ensure((a.ix.n_tiles + 1) * 8));
    a.state = ws[AW_STATE].as<unsigned long long>();
    a.kept = ws[AW_KEPT].as<uint64_t>();
    a.kept_base = ws[AW_KEPT_BASE].as<uint64_t>();
    unsigned long long state[ST_WORDS] = {};
    uint64_t* offs[1];
    DeliveredLength terms[1];
    size_t tmp_sums = 0, tmp_tiles_bytes = 0;
    const auto size = [&](size_t tmp_tiles, void** scan_tmp) -> zsw_error {
        // the per-record arrays hold as many records as pos_cap '>' can make
        a.rec_items = a.ix.pos_cap + 1;
        // hipcub counts its items in an int: the first round's estimate always fits (n_bytes <= 2^36), an exact count of '>' may not
        if (a.rec_items + 1 > (uint64_t)INT_MAX) return fail(ctx, ZSW_ERR_UNSUPPORTED, "fasta: more than 2^31 '>' per call: parse the file in chunks");
        ZSW_HIP(ctx, ws[AW_CODE].ensure(a.rec_items));
        ZSW_HIP(ctx, ws[AW_NAME_LEN].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[AW_BODY_LO].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[AW_NAME_OFF].ensure((a.rec_items + 1) * 8));
        ZSW_HIP(ctx, ws[AW_SEQ_OFF].ensure((a.rec_items + 1) * 8));
        a.code = ws[AW_CODE].as<uint8_t>();
        a.name_len = ws[AW_NAME_LEN].as<uint64_t>();
        a.body_lo = ws[AW_BODY_LO].as<uint64_t>();
        a.name_off = offs[0] = ws[AW_NAME_OFF].as<uint64_t>();
        a.seq_off = ws[AW_SEQ_OFF].as<uint64_t>();
        terms[0] = DeliveredLength{a.name_len, a.state + ST_DELIVERED};
        tmp_sums = 0;
        ZSW_HIP(ctx, delivered_sums(nullptr, &tmp_sums, terms, offs, 1, (int)(a.rec_items + 1), stream));
        tmp_tiles_bytes = tmp_tiles;  // the scan over the kept bytes has the index scan's shape
        ZSW_HIP(ctx, ws[AW_SCAN_TMP].ensure(std::max(tmp_tiles, tmp_sums) + 16));
        *scan_tmp = ws[AW_SCAN_TMP].p;
        return ZSW_OK;
    };
    const auto launch = [&](void* scan_tmp) -> zsw_error {
        const dim3 grid(grid_for(ctx, a.rec_items, FA_BLOCK_RECORDS));
        const dim3 tile_grid(grid_for(ctx, a.ix.n_tiles, FQ_TILE_WAVES));
        hipLaunchKernelGGL(fa_record_kernel, grid, dim3(REC_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(fa_plan_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, delivered_sums(scan_tmp, &tmp_sums, terms, offs, 1, (int)(a.rec_items + 1), stream));
        if (a.ix.n_tiles) {
            hipLaunchKernelGGL(fa_sequence_kernel<false>, tile_grid, dim3(TILE_BLOCK), 0, stream, a);
            ZSW_HIP(ctx, hipGetLastError());
            ZSW_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(scan_tmp, tmp_tiles_bytes, a.kept, const_cast<uint64_t*>(a.kept_base), (int)(a.ix.n_tiles + 1), stream));
            hipLaunchKernelGGL(fa_sequence_kernel<true>, tile_grid, dim3(TILE_BLOCK), 0, stream, a);
        }
        hipLaunchKernelGGL(fa_gather_kernel, grid, dim3(REC_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(fa_report_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        return ZSW_OK;
    };
    if (zsw_error e = run_rounds<ST_WORDS>(ctx, &a.ix, 64, a.state, state, "fasta: the '>' positions did not fit twice", size, launch, stream, '>')) return e;
    if (state[ST_BAD_START]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, bad_start);
    for (int k = 0; k < INFO_WORDS; ++k) out_info[k] = state[ST_INFO + k];
    if (sizing) return ZSW_OK;
    if (!state[ST_WRITTEN]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a capacity is too small; required sizes returned in out_info");
    if (host) {
        const size_t off_bytes = (out_info[INFO_RECORDS] + 1) * 8;
        const size_t used[4] = {(size_t)out_info[INFO_BASES], off_bytes, (size_t)out_info[INFO_NAME_BYTES], off_bytes};
        if (zsw_error e = copy_down(ctx, downs, used, 4, stream)) return e;
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
