// zsw_fastq.hip — zsw_fastq_parse_batch (include/zoe_sw.h): FASTQ bytes in device memory to the arrays zsw_batch and zsw_sam_fields
// take — bases and qualities back to back with offsets, names with qname_offsets. The rules are zsw_fastq.hpp (shared with
// tests/models/fastq_parse.cpp); the newline index is zsw_text.hip; the state block, the init and plan kernels, the sums and the
// rounds are zsw_text_dev.hpp. This file is the records: the wavefront behind the header's Io, their launches and the entry point.
//
// Launches, all on the caller's stream, with no host step between them:
//   init      the state block (lowest failing record, min / max length)
//   index     zsw_text.hip: newlines per tile, their exclusive sum, the position of every newline at its rank
//   records   one wavefront per record: parse_record -> code, name length, sequence length; an atomicMin of the lowest failing index
//   plan      one thread: delivered = min(records, lowest failing index)
//   scan x 2  exclusive sums of the name and sequence lengths of the delivered prefix -> offsets
//   gather    one wavefront per record: offsets, name, bases, qualities; nothing if a capacity is too small; min / max length
//   report    one thread: the nine words of out_info
// then one copy of the report and one synchronisation. A minimum and a maximum are the only atomics: every output is the same on
// every run. The number of newlines is not known to the host when the workspace is sized: 8 bytes per 16 bytes of text are provided
// (lines of 15 bytes and a newline on average); a denser text is found out by the report and the launches from `positions` on run
// once more with the exact size — the one case of a second synchronisation, and the context keeps the larger workspace.
#include "zsw_text_dev.hpp"

#include "zsw_fastq.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::fastq;

static_assert(ZSW_FASTQ_FINAL == F_FINAL && ZSW_FASTQ_NAME_TO_BLANK == F_NAME_TO_BLANK, "zsw_fastq.hpp mirrors the header's flags");
static_assert(ZSW_FASTQ_INFO_WORDS == INFO_WORDS && ZSW_FASTQ_INFO_MAX_LEN == INFO_MAX_LEN && ZSW_FASTQ_INFO_CONSUMED == INFO_CONSUMED,
              "zsw_fastq.hpp mirrors the header's report");
static_assert(ZSW_FASTQ_INVALID_QUALITY == INVALID_QUALITY && ZSW_FASTQ_MISSING_AT == MISSING_AT, "zsw_fastq.hpp mirrors the header's codes");

namespace {

enum { FW_CODE = 0, FW_NAME_LEN, FW_SEQ_LEN, FW_NAME_OFF, FW_SEQ_OFF, FW_SCAN_TMP, FW_STATE, FW_BASES, FW_QUALS, FW_OFFSETS, FW_QNAMES, FW_QOFF, FW_N };

constexpr int ST_WORDS = ST_INFO + INFO_WORDS;

struct FqArgs {
    IndexArgs ix;             // the newline index: text, n_bytes, head, tiles, pos, pos_cap
    int flags;
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

// The wavefront behind the header's walk
struct WaveIo : WaveSweeps<WaveIo> {
    int lane;
    const uint8_t* text;
    const uint64_t* pos_in;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const { return text[p]; }
    __device__ __forceinline__ uint64_t sweep_blank(uint64_t lo, uint64_t n) const { return sweep_first(lo, n, [](uint8_t c) { return is_blank(c); }); }
};
__device__ __forceinline__ bool fq_text(const FqArgs& a, Text* t, uint64_t* n_rec) { return text_of<n_records>(a.ix, a.flags, a.rec_items, t, n_rec); }

__global__ __launch_bounds__(REC_BLOCK) void fq_record_kernel(FqArgs a) {
    const int lane = threadIdx.x & 63;
    Text t;
    uint64_t n_rec;
    if (!fq_text(a, &t, &n_rec)) return;
    WaveIo io{{}, lane, a.ix.text, a.ix.pos};
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

// the lengths of the delivered prefix, 0 behind it: what the two offset scans sum
struct DeliveredLength {
    const uint64_t* len;
    const unsigned long long* delivered;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i < *delivered ? len[i] : 0; }
};

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
    WaveIo io{{}, lane, a.ix.text, a.ix.pos};
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
        wave_copy(a.out_bases + s0, a.ix.text + R.seq_lo, s_len, lane);
        if (a.out_quals) wave_copy(a.out_quals + s0, a.ix.text + R.qual_lo, s_len, lane);
        if (lane == 0) a.out_offsets[r] = s0;
        if (want_names) {
            const uint64_t n0 = uni(a.name_off[r]), n_len = uni(a.name_off[r + 1]) - n0;
            if (R.name_lo + n_len > t.n_bytes || n0 + n_len > a.name_cap) continue;
            wave_copy(a.out_qnames + n0, a.ix.text + R.name_lo, n_len, lane);
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
    WaveIo io{{}, 0, a.ix.text, a.ix.pos};
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

}  // namespace

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
    const Span spans[6] = {{text, n_bytes}, {out_bases, base_cap}, {out_quals, base_cap}, {out_offsets, (record_cap + 1) * 8}, {out_qnames, name_cap},
                           {out_qname_offsets, (record_cap + 1) * 8}};
    if (const int i = first_overlap(spans, 6); i >= 0) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, i ? "output arrays overlap" : "an output array overlaps the text");
    const bool host = mem == ZSW_MEM_HOST;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->fq_ws;
    static_assert(FW_N <= sizeof(ctx->fq_ws) / sizeof(ctx->fq_ws[0]), "zsw_context::fq_ws holds every buffer");
    FqArgs a{};
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
    if (zsw_error e = index_prepare(ctx, &a.ix, text, n_bytes, host, stream)) return e;
    const bool staged = host && !sizing;  // the outputs are formed in workspace no larger than the bounds that always suffice
    if (staged) {
        a.base_cap = std::min<uint64_t>(base_cap, n_bytes / 2);
        a.name_cap = std::min<uint64_t>(name_cap, n_bytes);
        a.record_cap = std::min<uint64_t>(record_cap, n_bytes / 8 + 1);
    }
    Down downs[5] = {{FW_BASES, a.base_cap, (void**)&a.out_bases}, {FW_QUALS, a.base_cap, (void**)&a.out_quals}, {FW_OFFSETS, (a.record_cap + 1) * 8, (void**)&a.out_offsets},
                     {FW_QNAMES, a.name_cap, (void**)&a.out_qnames}, {FW_QOFF, (a.record_cap + 1) * 8, (void**)&a.out_qname_offsets}};
    if (staged)
        if (zsw_error e = stage_down(ctx, ws, downs, 5)) return e;
    ZSW_HIP(ctx, ws[FW_STATE].ensure(ST_WORDS * 8));
    a.state = ws[FW_STATE].as<unsigned long long>();
    unsigned long long state[ST_WORDS] = {};
    uint64_t* offs[2];
    DeliveredLength terms[2];
    size_t tmp_sums = 0;
    const auto size = [&](size_t tmp_tiles, void** scan_tmp) -> zsw_error {
        // the per-record arrays hold ceil((newlines + 1) / 4) records: as many as pos_cap newlines can make
        a.rec_items = a.ix.pos_cap / 4 + 1;
        // hipcub counts its items in an int: the first round's estimate always fits (n_bytes <= 2^36), an exact count of newlines may not
        if (a.rec_items + 1 > (uint64_t)INT_MAX) return fail(ctx, ZSW_ERR_UNSUPPORTED, "fastq: more than 2^33 newlines per call: parse the file in chunks");
        ZSW_HIP(ctx, ws[FW_CODE].ensure(a.rec_items));
        ZSW_HIP(ctx, ws[FW_NAME_LEN].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[FW_SEQ_LEN].ensure(a.rec_items * 8));
        ZSW_HIP(ctx, ws[FW_NAME_OFF].ensure((a.rec_items + 1) * 8));
        ZSW_HIP(ctx, ws[FW_SEQ_OFF].ensure((a.rec_items + 1) * 8));
        a.code = ws[FW_CODE].as<uint8_t>();
        a.name_len = ws[FW_NAME_LEN].as<uint64_t>();
        a.seq_len = ws[FW_SEQ_LEN].as<uint64_t>();
        a.name_off = offs[0] = ws[FW_NAME_OFF].as<uint64_t>();
        a.seq_off = offs[1] = ws[FW_SEQ_OFF].as<uint64_t>();
        terms[0] = DeliveredLength{a.name_len, a.state + ST_DELIVERED};
        terms[1] = DeliveredLength{a.seq_len, a.state + ST_DELIVERED};
        tmp_sums = 0;
        ZSW_HIP(ctx, delivered_sums(nullptr, &tmp_sums, terms, offs, 2, (int)(a.rec_items + 1), stream));
        ZSW_HIP(ctx, ws[FW_SCAN_TMP].ensure(std::max(tmp_tiles, tmp_sums) + 16));
        *scan_tmp = ws[FW_SCAN_TMP].p;
        return ZSW_OK;
    };
    const auto launch = [&](void* scan_tmp) -> zsw_error {
        const dim3 grid(grid_for(ctx, a.rec_items, FQ_BLOCK_RECORDS));
        if (a.ix.n_tiles) hipLaunchKernelGGL(fq_record_kernel, grid, dim3(REC_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(plan_kernel<n_records>, dim3(1), dim3(1), 0, stream, a.ix, a.flags, a.rec_items, a.state);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, delivered_sums(scan_tmp, &tmp_sums, terms, offs, 2, (int)(a.rec_items + 1), stream));
        hipLaunchKernelGGL(fq_gather_kernel, grid, dim3(REC_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(fq_report_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        return ZSW_OK;
    };
    if (zsw_error e = run_rounds<ST_WORDS>(ctx, &a.ix, 16, a.state, state, "fastq: the newline positions did not fit twice", size, launch, stream)) return e;
    for (int k = 0; k < INFO_WORDS; ++k) out_info[k] = state[ST_INFO + k];
    if (sizing) return ZSW_OK;
    if (!state[ST_WRITTEN]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a capacity is too small; required sizes returned in out_info");
    if (host) {
        const size_t nb = out_info[INFO_BASES], off_bytes = (out_info[INFO_RECORDS] + 1) * 8;
        const size_t used[5] = {nb, nb, off_bytes, (size_t)out_info[INFO_NAME_BYTES], off_bytes};
        if (zsw_error e = copy_down(ctx, downs, used, 5, stream)) return e;
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
