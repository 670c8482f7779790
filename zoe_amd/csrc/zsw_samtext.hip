// zsw_samtext.hip — zsw_sam_parse_batch (include/zoe_sw.h): SAM text in device memory to the arrays zsw_annotate_batch,
// zsw_sam_batch and zsw_pileup_batch take — records with status and ciglets, and the reads as bases / quals / names with offsets.
// The rules are zsw_samtext.hpp (shared with tests/models/samtext_parse.cpp); the newline index is zsw_text.hip; the state block, the
// init and plan kernels, the sums and the rounds are zsw_text_dev.hpp. This file is the lines: the wavefront behind the header's Io
// with the members the SAM rules need, their launches and the entry point.
//
// Launches, all on the caller's stream, with no host step between them:
//   init      the state block (lowest failing line, min / max length)
//   index     zsw_text.hip: newlines per tile, their exclusive sum, the position of every newline at its rank
//   lines     one wavefront per line, the line's first SAM_WINDOW bytes staged in LDS: parse_line -> the line's record
//             (zsw_samtext.hpp, Line); an atomicMin of the lowest failing index
//   plan      one thread: delivered lines = min(lines, lowest failing index)
//   scan x 6  exclusive sums over the delivered lines: data lines (a line's record index), bases, name bytes, ciglets, mapped, coded
//   gather    one wavefront per delivered data line: bases, qualities, name, record, status, strand, parsed, and the CIGAR walked
//             once more with a sink that writes the merged ciglets at the line's place; nothing if a capacity is too small
//   report    one thread: the words of out_info
// then one copy of the report and one synchronisation. A minimum and a min / max are the only atomics. The workspace for the newline
// positions is sized for a line per 64 bytes; a denser text repeats the launches from the positions on, as in zsw_fastq.hip.
#include "zsw_text_dev.hpp"

#include "zsw_samtext.hpp"

using namespace zsw;
using namespace zsw::capi;
using namespace zsw::samtext;

static_assert(ZSW_SAMTEXT_FINAL == SF_FINAL && ZSW_SAMTEXT_QUAL_FORWARD == SF_QUAL_FORWARD, "zsw_samtext.hpp mirrors the header's flags");
static_assert(ZSW_SAMTEXT_INFO_WORDS == SI_WORDS && ZSW_SAMTEXT_INFO_MAX_LEN == SI_MAX_LEN && ZSW_SAMTEXT_INFO_CONSUMED == SI_CONSUMED &&
                  ZSW_SAMTEXT_INFO_CODED == SI_CODED,
              "zsw_samtext.hpp mirrors the header's report");
static_assert(ZSW_SAMTEXT_INVALID_QUALITY == SR_INVALID_QUALITY && ZSW_SAMREC_TOO_LARGE == SC_TOO_LARGE && ZSW_SAMREC_BIT_QUAL_LENGTH == SB_QUAL_LENGTH,
              "zsw_samtext.hpp mirrors the header's codes");
static_assert(sizeof(zsw_sam_parsed) == 24 && sizeof(zsw_alignment) == 40, "the layouts the header states");
static_assert((uint32_t)ZSW_STATUS_SOME == ST_SOME && (uint32_t)ZSW_STATUS_UNMAPPED == ST_UNMAPPED, "zsw_samtext.hpp mirrors zsw_status");

namespace {

enum { SW_LINES = 0, SW_REC_OFF, SW_SEQ_OFF, SW_NAME_OFF, SW_CIG_OFF, SW_MAP_OFF, SW_CODE_OFF, SW_SCAN_TMP, SW_STATE,
       SW_RNAME, SW_BASES, SW_QUALS, SW_OFFSETS, SW_QNAMES, SW_QOFF, SW_ALN, SW_STATUS, SW_INC, SW_OP, SW_STRAND, SW_PARSED, SW_N };

constexpr int ST_WORDS = ST_INFO + SI_WORDS;

enum { SUM_RECORDS = 0, SUM_BASES, SUM_NAMES, SUM_CIGLETS, SUM_MAPPED, SUM_CODED, SUM_N };

struct SamArgs {
    IndexArgs ix;             // the newline index: text, n_bytes, head, tiles, pos, pos_cap
    int flags;
    uint32_t rname_len, ref_len;
    const uint8_t* rname;     // device copy of the caller's RNAME, rname_len bytes
    uint64_t line_items;      // entries of the per-line arrays
    Line* lines;
    const uint64_t* sum[SUM_N];  // line_items + 1 each
    unsigned long long* state;
    uint8_t *out_bases, *out_quals, *out_qnames, *out_status, *out_op, *out_strand;
    uint64_t *out_offsets, *out_qname_offsets;
    zsw_alignment* out_aln;
    uint32_t* out_inc;
    zsw_sam_parsed* out_parsed;
    uint64_t base_cap, name_cap, ciglet_cap, record_cap;
    int write;                // 0: the sizing call
};

constexpr uint32_t LINE_BLOCK = FQ_G * SAM_BLOCK_LINES;

constexpr uint32_t SAM_WINDOW = 1024;  // bytes of a line that its wavefront keeps in LDS
typedef __attribute__((address_space(3))) uint8_t lds_u8;

// The wavefront behind the walk of zsw_samtext.hpp. The walk reads most bytes of a line one at a time, each load waiting for the
// one before it; stage() copies the head of the line into the wavefront's LDS window with consecutive lanes on consecutive bytes,
// and byte() answers from there. Bytes outside the window (a line longer than SAM_WINDOW, or no window at all) come from the text.
// newline(), sweep_utf8, sweep_quality and the first match by ballot are WaveSweeps' (zsw_text_dev.hpp), over this byte().
struct SamIo : WaveSweeps<SamIo> {
    int lane;
    const uint8_t* text;
    const uint64_t* pos_in;
    const uint8_t* rname;
    lds_u8* win;            // SAM_WINDOW bytes of LDS (an LDS pointer by type: ds loads, not flat ones)
    bool has_win;
    uint64_t win_lo, win_n;
    CigLane mine;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const {
        const uint64_t d = p - win_lo;
        return d < win_n ? win[d] : text[p];
    }
    __device__ __forceinline__ void stage(uint64_t lo, uint64_t hi) {
        if (!has_win) return;
        const uint64_t n = hi - lo < (uint64_t)SAM_WINDOW ? hi - lo : (uint64_t)SAM_WINDOW;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the reads of the line before are done
        __builtin_amdgcn_wave_barrier();
        for (uint64_t j = (uint32_t)lane; j < n; j += FQ_G) win[j] = text[lo + j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        win_lo = lo;
        win_n = n;
    }
    __device__ __forceinline__ unsigned long long mask_byte(uint64_t lo, uint64_t n, uint8_t c) const {
        return __ballot((uint64_t)(uint32_t)lane < n && byte(lo + (uint32_t)lane) == c);
    }
    __device__ __forceinline__ uint64_t sweep_byte(uint64_t lo, uint64_t n, uint8_t c) const { return sweep_first(lo, n, [c](uint8_t b) { return b == c; }); }
    __device__ __forceinline__ bool sweep_differs(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (uint64_t j = (uint32_t)lane; j < n; j += FQ_G) bad |= byte(lo + j) != rname[j];
        return __ballot(bad) != 0;
    }
    __device__ __forceinline__ unsigned long long cig_sweep(uint64_t c_lo, uint64_t lo, uint64_t n) {
        const bool op = (uint64_t)(uint32_t)lane < n && !is_digit(byte(lo + (uint32_t)lane));
        if (op) mine = cig_lane(*this, c_lo, lo + (uint32_t)lane);
        return __ballot(op);
    }
    __device__ __forceinline__ CigLane cig_pick(uint32_t j) const {
        CigLane L;
        L.inc = (uint64_t)(uint32_t)__shfl((int)(uint32_t)mine.inc, (int)j, FQ_G) | ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(mine.inc >> 32), (int)j, FQ_G) << 32);
        L.bits = (uint32_t)__shfl((int)mine.bits, (int)j, FQ_G);
        return L;
    }
};

__device__ __forceinline__ SamIo sam_io(const SamArgs& a, int lane, uint8_t* win = nullptr) {  // win: a __shared__ array
    SamIo io;
    io.lane = lane;
    io.text = a.ix.text;
    io.pos_in = a.ix.pos;
    io.rname = a.rname;
    io.win = (lds_u8*)win;
    io.has_win = win != nullptr;
    io.win_lo = io.win_n = 0;
    io.mine = CigLane{0, 0};
    return io;
}

__device__ __forceinline__ bool st_text(const SamArgs& a, Text* t, uint64_t* lines) { return text_of<n_lines>(a.ix, a.flags, a.line_items, t, lines); }

// Four waves per SIMD: the pass is bound by the latency of its dependent loads (15.6 ms at two waves, 10.6 ms at four, 2 M lines;
// DESIGN.md 4.11), and 128 registers cost 96 bytes of spills per lane.
__global__ __launch_bounds__(LINE_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void st_line_kernel(SamArgs a) {
    const int lane = threadIdx.x & 63;
    Text t;
    uint64_t lines;
    if (!st_text(a, &t, &lines)) return;
    __shared__ uint8_t window[SAM_BLOCK_LINES][SAM_WINDOW];
    SamIo io = sam_io(a, lane, window[threadIdx.x >> 6]);
    const uint64_t stride = (uint64_t)gridDim.x * SAM_BLOCK_LINES;
    uint64_t first_bad = ~0ull;
    for (uint64_t L = (uint64_t)blockIdx.x * SAM_BLOCK_LINES + uni((uint32_t)(threadIdx.x >> 6)); L < lines; L += stride) {
        const Line R = parse_line(io, t, L, a.rname_len);
        if (lane == 0) a.lines[L] = R;
        if (R.code && L < first_bad) first_bad = L;
    }
    if (lane == 0 && first_bad != ~0ull) atomicMin(&a.state[ST_FIRST_BAD], (unsigned long long)first_bad);
}

// what a delivered line adds to sum `which`, 0 behind the delivered lines and for header lines
struct LineTerm {
    const Line* lines;
    const unsigned long long* delivered;
    int which;
    __host__ __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        if (i >= *delivered) return 0;
        const Line& l = lines[i];
        if (l.kind != KIND_DATA) return 0;
        switch (which) {
            case SUM_RECORDS: return 1;
            case SUM_BASES: return l.seq_len;
            case SUM_NAMES: return l.name_len;
            case SUM_CIGLETS: return l.n_ciglets;
            case SUM_MAPPED: return l.status == ST_SOME ? 1 : 0;
            default: return l.rec_code ? 1 : 0;
        }
    }
};

struct WriteSink {
    uint32_t* inc;
    uint8_t* op;
    uint64_t n;
    int lane;
    __device__ __forceinline__ void put(uint64_t k, uint64_t i, uint32_t o) const {
        if (lane == 0 && k < n) {
            inc[k] = (uint32_t)i;
            op[k] = (uint8_t)o;
        }
    }
};

__global__ __launch_bounds__(LINE_BLOCK) void st_gather_kernel(SamArgs a) {
    const int lane = threadIdx.x & 63;
    if (a.state[ST_OVERFLOW]) return;
    Text t;
    uint64_t lines;
    if (!st_text(a, &t, &lines)) return;
    const uint64_t d = uni((uint64_t)a.state[ST_DELIVERED]);
    const uint64_t records = uni(a.sum[SUM_RECORDS][d]), bases = uni(a.sum[SUM_BASES][d]), names = uni(a.sum[SUM_NAMES][d]), ciglets = uni(a.sum[SUM_CIGLETS][d]);
    const bool want_names = a.out_qnames != nullptr;
    const bool write = a.write && records <= a.record_cap && bases <= a.base_cap && (!want_names || names <= a.name_cap) && ciglets <= a.ciglet_cap;
    SamIo io = sam_io(a, lane);
    const uint32_t wave = uni((uint32_t)(threadIdx.x >> 6));
    if (write && blockIdx.x == 0 && wave == 0 && lane == 0) {
        a.out_offsets[records] = bases;
        if (want_names) a.out_qname_offsets[records] = names;
        a.state[ST_WRITTEN] = 1;
    }
    const uint64_t stride = (uint64_t)gridDim.x * SAM_BLOCK_LINES;
    uint64_t lo = ~0ull, hi = 0;
    bool any = false;
    for (uint64_t L = (uint64_t)blockIdx.x * SAM_BLOCK_LINES + wave; L < d; L += stride) {
        if (uni(a.lines[L].kind) != KIND_DATA) continue;
        const Line R = a.lines[L];
        const uint64_t s_len = uni(R.seq_len), n_len = uni(R.name_len);
        any = true;
        lo = s_len < lo ? s_len : lo;
        hi = s_len > hi ? s_len : hi;
        if (!write) continue;
        const uint64_t r = uni(a.sum[SUM_RECORDS][L]), s0 = uni(a.sum[SUM_BASES][L]), n0 = uni(a.sum[SUM_NAMES][L]), c0 = uni(a.sum[SUM_CIGLETS][L]);
        const uint64_t seq_lo = uni(R.seq_lo), qual_lo = uni(R.qual_lo), name_lo = uni(R.name_lo), cig_lo = uni(R.cig_lo), cig_len = uni(R.cig_len);
        const uint32_t n_cig = uni(R.n_ciglets), flag = uni(R.flag);
        // the line pass found these inside the line; they are asked once more, in 64 bits, before the loads and the stores
        if (seq_lo + s_len > t.n_bytes || name_lo + n_len > t.n_bytes || cig_lo + cig_len > t.n_bytes || r >= a.record_cap || s0 + s_len > a.base_cap ||
            c0 + n_cig > a.ciglet_cap)
            continue;
        wave_copy(a.out_bases + s0, a.ix.text + seq_lo, s_len, lane);
        if (a.out_quals) {
            const bool fill = uni(R.qual_fill) != 0 || qual_lo + s_len > t.n_bytes;
            const bool back = (a.flags & SF_QUAL_FORWARD) && (flag & 16u);
            for (uint64_t j = (uint32_t)lane; j < s_len; j += FQ_G) a.out_quals[s0 + j] = fill ? (uint8_t)'!' : a.ix.text[qual_lo + (back ? s_len - 1u - j : j)];
        }
        if (want_names && n0 + n_len <= a.name_cap) {
            wave_copy(a.out_qnames + n0, a.ix.text + name_lo, n_len, lane);
            if (lane == 0) a.out_qname_offsets[r] = n0;
        }
        if (lane == 0) {
            const bool some = R.status == ST_SOME;
            zsw_alignment A{};
            if (some) {
                A.score = R.score;
                A.ref_start = R.ref_start;
                A.ref_end = R.ref_end;
                A.query_start = R.query_start;
                A.query_end = R.query_end;
                A.ref_len = a.ref_len;
                A.query_len = (uint32_t)s_len;
                A.n_ciglets = n_cig;
                A.ciglet_offset = c0;
            }
            a.out_offsets[r] = s0;
            a.out_aln[r] = A;
            a.out_status[r] = (uint8_t)R.status;
            if (a.out_strand) a.out_strand[r] = (flag & 16u) ? 1 : 0;
            if (a.out_parsed) {
                zsw_sam_parsed P;
                P.pos = R.pos;
                P.line = L;
                P.flag = (uint16_t)flag;
                P.mapq = (uint8_t)R.mapq;
                P.code = (uint8_t)R.rec_code;
                P.bits = R.bits;
                a.out_parsed[r] = P;
            }
        }
        if (n_cig) {
            WriteSink sink{a.out_inc + c0, a.out_op + c0, n_cig, lane};
            walk_cigar(io, cig_lo, cig_lo + cig_len, sink);
        }
    }
    if (lane == 0 && any) {
        atomicMin(&a.state[ST_MIN], (unsigned long long)lo);
        atomicMax(&a.state[ST_MAX], (unsigned long long)hi);
    }
}

__global__ void st_report_kernel(SamArgs a) {
    unsigned long long* info = a.state + ST_INFO;
    Text t;
    uint64_t lines;
    if (a.state[ST_OVERFLOW] || !st_text(a, &t, &lines)) return;
    SamIo io = sam_io(a, 0);
    const uint64_t d = a.state[ST_DELIVERED];
    const uint64_t records = a.sum[SUM_RECORDS][d];
    info[SI_RECORDS] = records;
    info[SI_HEADERS] = d - records;
    info[SI_BASES] = a.sum[SUM_BASES][d];
    info[SI_NAME_BYTES] = a.sum[SUM_NAMES][d];
    info[SI_CIGLETS] = a.sum[SUM_CIGLETS][d];
    info[SI_CONSUMED] = line_start(io, t, d);
    if (d < lines) {
        info[SI_ERROR] = a.lines[d].code;
        info[SI_ERROR_LINE] = d;
        info[SI_ERROR_OFFSET] = line_start(io, t, d);
    }
    info[SI_MAPPED] = a.sum[SUM_MAPPED][d];
    info[SI_CODED] = a.sum[SUM_CODED][d];
    info[SI_MIN_LEN] = records ? a.state[ST_MIN] : 0;
    info[SI_MAX_LEN] = a.state[ST_MAX];
}

}  // namespace

extern "C" zsw_error zsw_sam_parse_batch(zsw_context* ctx, const uint8_t* text, uint64_t n_bytes, zsw_mem mem, int flags, const char* rname, uint32_t rname_len,
                                         uint32_t ref_len, const void* out_, uint64_t* out_info, void* stream_) {
    if (!ctx) return ZSW_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx);
    hipStream_t stream = (hipStream_t)stream_;
    if (!out_info || !out_ || (n_bytes && !text)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~SF_ALL) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown sam text flag");
    if (mem != ZSW_MEM_HOST && mem != ZSW_MEM_DEVICE) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "unknown mem");
    if ((rname == nullptr) != (rname_len == 0) || rname_len > 255u) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "rname and rname_len go together, 1..255 bytes");
    const zsw_sam_parse_out o = *static_cast<const zsw_sam_parse_out*>(out_);
    const bool sizing = !o.bases && !o.quals && !o.offsets && !o.qnames && !o.qname_offsets && !o.aln && !o.status && !o.inc && !o.op && !o.strand && !o.parsed &&
                        !o.base_cap && !o.name_cap && !o.ciglet_cap && !o.record_cap;
    if (!sizing && (!o.bases || !o.offsets || !o.aln || !o.status || !o.inc || !o.op))
        return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "null bases / offsets / aln / status / inc / op outside the sizing call");
    if ((o.qnames == nullptr) != (o.qname_offsets == nullptr)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "qnames and qname_offsets go together");
    if (n_bytes > (1ull << 36)) return fail(ctx, ZSW_ERR_UNSUPPORTED, "more than 2^36 bytes per call: parse the file in chunks");
    if (o.record_cap >= (1ull << 56) || o.ciglet_cap >= (1ull << 60)) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "record_cap / ciglet_cap");
    const bool want_names = o.qnames != nullptr;
    const uint64_t name_cap = want_names ? o.name_cap : 0;
    const Span spans[12] = {{text, n_bytes}, {o.bases, o.base_cap}, {o.quals, o.base_cap}, {o.offsets, (o.record_cap + 1) * 8}, {o.qnames, name_cap},
                            {o.qname_offsets, (o.record_cap + 1) * 8}, {o.aln, o.record_cap * sizeof(zsw_alignment)}, {o.status, o.record_cap}, {o.inc, o.ciglet_cap * 4},
                            {o.op, o.ciglet_cap}, {o.strand, o.record_cap}, {o.parsed, o.record_cap * sizeof(zsw_sam_parsed)}};
    if (const int i = first_overlap(spans, 12); i >= 0) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, i ? "output arrays overlap" : "an output array overlaps the text");
    const bool host = mem == ZSW_MEM_HOST;
    ZSW_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf* ws = ctx->samtext_ws;
    static_assert(SW_N <= sizeof(ctx->samtext_ws) / sizeof(ctx->samtext_ws[0]), "zsw_context::samtext_ws holds every buffer");
    SamArgs a{};
    a.flags = flags;
    a.rname_len = rname_len;
    a.ref_len = ref_len;
    a.out_bases = o.bases;
    a.out_quals = o.quals;
    a.out_offsets = o.offsets;
    a.out_qnames = o.qnames;
    a.out_qname_offsets = o.qname_offsets;
    a.out_aln = o.aln;
    a.out_status = o.status;
    a.out_inc = o.inc;
    a.out_op = o.op;
    a.out_strand = o.strand;
    a.out_parsed = static_cast<zsw_sam_parsed*>(o.parsed);
    a.base_cap = o.base_cap;
    a.name_cap = name_cap;
    a.ciglet_cap = o.ciglet_cap;
    a.record_cap = o.record_cap;
    a.write = sizing ? 0 : 1;
    if (rname_len) {
        ZSW_HIP(ctx, ws[SW_RNAME].ensure(256));
        ZSW_HIP(ctx, hipMemcpyAsync(ws[SW_RNAME].p, rname, rname_len, hipMemcpyHostToDevice, stream));
        a.rname = ws[SW_RNAME].as<uint8_t>();
    }
    if (zsw_error e = index_prepare(ctx, &a.ix, text, n_bytes, host, stream)) return e;
    const bool staged = host && !sizing;  // the outputs are formed in workspace no larger than the bounds that always suffice
    if (staged) {
        a.base_cap = std::min<uint64_t>(o.base_cap, n_bytes);
        a.name_cap = std::min<uint64_t>(name_cap, n_bytes);
        a.ciglet_cap = std::min<uint64_t>(o.ciglet_cap, n_bytes / 2);
        a.record_cap = std::min<uint64_t>(o.record_cap, n_bytes / 14 + 1);
    }
    constexpr int N_DOWN = 11;
    Down downs[N_DOWN] = {{SW_BASES, a.base_cap, (void**)&a.out_bases}, {SW_QUALS, a.base_cap, (void**)&a.out_quals}, {SW_OFFSETS, (a.record_cap + 1) * 8, (void**)&a.out_offsets},
                          {SW_QNAMES, a.name_cap, (void**)&a.out_qnames}, {SW_QOFF, (a.record_cap + 1) * 8, (void**)&a.out_qname_offsets},
                          {SW_ALN, (a.record_cap + 1) * sizeof(zsw_alignment), (void**)&a.out_aln}, {SW_STATUS, a.record_cap, (void**)&a.out_status},
                          {SW_STRAND, a.record_cap, (void**)&a.out_strand}, {SW_PARSED, (a.record_cap + 1) * sizeof(zsw_sam_parsed), (void**)&a.out_parsed},
                          {SW_INC, a.ciglet_cap * 4, (void**)&a.out_inc}, {SW_OP, a.ciglet_cap, (void**)&a.out_op}};
    if (staged)
        if (zsw_error e = stage_down(ctx, ws, downs, N_DOWN)) return e;
    ZSW_HIP(ctx, ws[SW_STATE].ensure(ST_WORDS * 8));
    a.state = ws[SW_STATE].as<unsigned long long>();
    unsigned long long state[ST_WORDS] = {};
    uint64_t* sums[SUM_N];
    LineTerm terms[SUM_N];
    size_t tmp_sums = 0;
    const auto size = [&](size_t tmp_tiles, void** scan_tmp) -> zsw_error {
        a.line_items = a.ix.pos_cap + 1;  // the lines that pos_cap newlines can make
        // hipcub counts its items in an int
        if (a.line_items + 1 > (uint64_t)INT_MAX) return fail(ctx, ZSW_ERR_UNSUPPORTED, "sam text: more than 2^31 lines per call: parse the file in chunks");
        ZSW_HIP(ctx, ws[SW_LINES].ensure(a.line_items * sizeof(Line)));
        a.lines = ws[SW_LINES].as<Line>();
        for (int k = 0; k < SUM_N; ++k) {
            ZSW_HIP(ctx, ws[SW_REC_OFF + k].ensure((a.line_items + 1) * 8));
            a.sum[k] = sums[k] = ws[SW_REC_OFF + k].as<uint64_t>();
            terms[k] = LineTerm{a.lines, a.state + ST_DELIVERED, k};
        }
        tmp_sums = 0;
        ZSW_HIP(ctx, delivered_sums(nullptr, &tmp_sums, terms, sums, SUM_N, (int)(a.line_items + 1), stream));
        ZSW_HIP(ctx, ws[SW_SCAN_TMP].ensure(std::max(tmp_tiles, tmp_sums) + 16));
        *scan_tmp = ws[SW_SCAN_TMP].p;
        return ZSW_OK;
    };
    const auto launch = [&](void* scan_tmp) -> zsw_error {
        const dim3 grid(grid_for(ctx, a.line_items, SAM_BLOCK_LINES));
        if (a.ix.n_tiles) hipLaunchKernelGGL(st_line_kernel, grid, dim3(LINE_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(plan_kernel<n_lines>, dim3(1), dim3(1), 0, stream, a.ix, a.flags, a.line_items, a.state);
        ZSW_HIP(ctx, hipGetLastError());
        ZSW_HIP(ctx, delivered_sums(scan_tmp, &tmp_sums, terms, sums, SUM_N, (int)(a.line_items + 1), stream));
        hipLaunchKernelGGL(st_gather_kernel, grid, dim3(LINE_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(st_report_kernel, dim3(1), dim3(1), 0, stream, a);
        ZSW_HIP(ctx, hipGetLastError());
        return ZSW_OK;
    };
    if (zsw_error e = run_rounds<ST_WORDS>(ctx, &a.ix, 64, a.state, state, "sam text: the newline positions did not fit twice", size, launch, stream)) return e;
    for (int k = 0; k < SI_WORDS; ++k) out_info[k] = state[ST_INFO + k];
    if (sizing) return ZSW_OK;
    if (!state[ST_WRITTEN]) return fail(ctx, ZSW_ERR_INVALID_ARGUMENT, "a capacity is too small; required sizes returned in out_info");
    if (host) {
        const size_t n = out_info[SI_RECORDS], nb = out_info[SI_BASES], nc = out_info[SI_CIGLETS], off_bytes = (n + 1) * 8;
        const size_t used[N_DOWN] = {nb, nb, off_bytes, (size_t)out_info[SI_NAME_BYTES], off_bytes, n * sizeof(zsw_alignment), n, n, n * sizeof(zsw_sam_parsed), nc * 4, nc};
        if (zsw_error e = copy_down(ctx, downs, used, N_DOWN, stream)) return e;
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
    }
    return ZSW_OK;
}
