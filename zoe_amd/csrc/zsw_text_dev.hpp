// zsw_text_dev.hpp — what zsw_fastq.hip and zsw_samtext.hip build their calls from, around the one step that is their own (records
// / lines). Not installed. Three parts:
//   (1) the newline index (zsw_text.hip, compiled once): IndexArgs, index_prepare, index_scan_bytes, index_launch, grid_for; its
//       buffers are zsw_context::text_ws, one set for both calls;
//   (2) the wavefront behind the Io of zsw_text.hpp: WaveSweeps, the sweeps in terms of the derived Io's byte();
//   (3) the pipeline, shared as text: the state block, its init and plan kernels, text_of, the sums over the delivered prefix,
//       and run_rounds — estimate the newlines, launch, read the state, once more from `positions` with the exact size.
#pragma once
#include <limits.h>

#include <hipcub/hipcub.hpp>

#include "zsw_context.hpp"
#include "zsw_text.hpp"
#include "zsw_wave.hpp"

namespace zsw {
namespace text {

// ---- (1) the newline index ---------------------------------------------------------------------------------------------------
enum { TW_TEXT = 0, TW_TILE_COUNTS, TW_TILE_BASE, TW_POS, TW_N };  // zsw_context::text_ws

struct IndexArgs {
    const uint8_t* text;
    uint64_t n_bytes;
    uint32_t head;              // address of text & 15
    uint64_t n_tiles;
    uint64_t* tile_counts;      // n_tiles + 1 (the last one 0)
    const uint64_t* tile_base;  // their exclusive sum
    uint64_t* pos;              // position of newline k, k < pos_cap
    uint64_t pos_cap;
};

uint32_t grid_for(const zsw_context* ctx, uint64_t items, uint32_t per_block);
// text, n_bytes, head, n_tiles, tile_counts, tile_base of *ix; the text of a host call crosses here (text_ws[TW_TEXT])
zsw_error index_prepare(zsw_context* ctx, IndexArgs* ix, const uint8_t* text, uint64_t n_bytes, bool host, hipStream_t stream);
// The newline index of ix.text on `stream`: with `count` the newlines per tile and their exclusive sum (ix.tile_base[ix.n_tiles] =
// how many there are), then the position of every newline at its rank, as far as pos_cap reaches. scan_tmp: index_scan_bytes. A
// caller whose workspace for the positions was an estimate finds tile_base[n_tiles] > pos_cap on the device, and calls once more
// without `count` and with the exact size (run_rounds).
hipError_t index_scan_bytes(const IndexArgs& ix, size_t* bytes, hipStream_t stream);
// byte: '\n', or '>' for the index of zsw_fasta_parse_batch's record delimiters (the same sweep, instantiated for that byte).
hipError_t index_launch(const zsw_context* ctx, const IndexArgs& ix, bool count, void* scan_tmp, size_t scan_bytes, hipStream_t stream, uint8_t byte = '\n');

using namespace zsw::wave;

// ---- (2) the wavefront behind the Io ------------------------------------------------------------------------------------------
// Lane k takes bytes k, k + FQ_G, ..; a ballot gives every lane the answer. D: the Io, with lane, pos_in and byte().
template <class D>
struct WaveSweeps {
    __device__ __forceinline__ const D& io() const { return *static_cast<const D*>(this); }
    __device__ __forceinline__ uint64_t newline(uint64_t rank) const { return uni(io().pos_in[rank]); }
    __device__ __forceinline__ bool sweep_utf8(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (uint64_t j = (uint32_t)io().lane; j < n; j += FQ_G) bad |= utf8_bad_at(io(), lo, n, j);
        return __ballot(bad) != 0;
    }
    __device__ __forceinline__ bool sweep_quality(uint64_t lo, uint64_t n) const {
        bool bad = false;
        for (uint64_t j = (uint32_t)io().lane; j < n; j += FQ_G) bad |= !quality_ok(io().byte(lo + j));
        return __ballot(bad) != 0;
    }
    // the lowest j < n with match(byte(lo + j)), else n
    template <class Match>
    __device__ __forceinline__ uint64_t sweep_first(uint64_t lo, uint64_t n, Match match) const {
        for (uint64_t j0 = 0; j0 < n; j0 += FQ_G) {
            const uint64_t j = j0 + (uint32_t)io().lane;
            const unsigned long long m = __ballot(j < n && match(io().byte(lo + j)));
            if (m) return j0 + (uint64_t)__builtin_ctzll(m);
        }
        return n;
    }
};

// ---- (3) the pipeline ----------------------------------------------------------------------------------------------------------
// the state block: what the launches hand each other, then the call's report words
enum { ST_FIRST_BAD = 0, ST_MIN, ST_MAX, ST_DELIVERED, ST_NEWLINES, ST_OVERFLOW, ST_WRITTEN, ST_INFO };

typedef uint64_t (*ItemsOf)(const Text&, bool);  // n_records, n_lines: the items these newlines make

template <int WORDS>
__global__ void state_init_kernel(unsigned long long* state) {
    for (int k = 0; k < WORDS; ++k) state[k] = 0;
    state[ST_FIRST_BAD] = ~0ull;
    state[ST_MIN] = ~0ull;
}

// what every later launch first asks: how many newlines, how many items; false: the positions did not fit, nothing is done
template <ItemsOf ITEMS>
__device__ __forceinline__ bool text_of(const IndexArgs& ix, int flags, uint64_t items_cap, Text* t, uint64_t* n) {
    t->n_bytes = ix.n_bytes;
    t->n_newlines = ix.n_tiles ? uni(ix.tile_base[ix.n_tiles]) : 0;
    t->flags = flags;
    if (t->n_newlines > ix.pos_cap) return false;
    const bool last_nl = ix.n_bytes ? uni((uint32_t)ix.text[ix.n_bytes - 1]) == '\n' : true;
    *n = ITEMS(*t, last_nl);
    return *n <= items_cap;  // holds by the sizes the entry point gives the arrays
}

// one thread: delivered = min(items, lowest failing index)
template <ItemsOf ITEMS>
__global__ void plan_kernel(IndexArgs ix, int flags, uint64_t items_cap, unsigned long long* state) {
    Text t;
    uint64_t n;
    state[ST_NEWLINES] = ix.n_tiles ? ix.tile_base[ix.n_tiles] : 0;
    if (!text_of<ITEMS>(ix, flags, items_cap, &t, &n)) {
        state[ST_OVERFLOW] = 1;
        state[ST_DELIVERED] = 0;
        return;
    }
    const uint64_t fb = state[ST_FIRST_BAD];
    state[ST_DELIVERED] = fb < n ? fb : n;
}

// Exclusive sums over `items` entries of terms[k](i) — a call's functor of "what item i of the delivered prefix adds, else 0" —
// to out[k]. tmp == nullptr: *tmp_bytes = the scratch the sums need, nothing is launched.
template <class Term>
hipError_t delivered_sums(void* tmp, size_t* tmp_bytes, const Term* terms, uint64_t* const* out, int n_sums, int items, hipStream_t stream) {
    size_t most = 0;
    for (int k = 0; k < n_sums; ++k) {
        const hipcub::TransformInputIterator<uint64_t, Term, hipcub::CountingInputIterator<uint64_t>> in(hipcub::CountingInputIterator<uint64_t>(0), terms[k]);
        size_t bytes = *tmp_bytes;
        const hipError_t e = hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out[k], items, stream);
        if (e != hipSuccess) return e;
        most = std::max(most, bytes);
    }
    if (!tmp) *tmp_bytes = most;
    return hipSuccess;
}

// The rounds of a parse call over the prepared *ix. pos_per_bytes: a newline per so many bytes is what the first round provides
// for. Per round, in this order: the positions are sized, size(tiles_tmp, &scan_tmp) sizes the call's per-item arrays for
// ix->pos_cap and gives the scans' scratch (tiles_tmp bytes at least); the state is initialised; the index is launched (round 0:
// with the counts); launch() launches everything behind the index; the state is copied to state[0 .. WORDS) and the stream is
// synchronised — the one synchronisation of a device call —; a text denser than the estimate goes once more, from the positions
// on, with the exact size. twice: the error text of a second overflow.
template <int WORDS, class Size, class Launch>
zsw_error run_rounds(zsw_context* ctx, IndexArgs* ix, uint64_t pos_per_bytes, unsigned long long* d_state, unsigned long long* state, const char* twice, Size size,
                     Launch launch, hipStream_t stream, uint8_t byte = '\n') {
    using namespace zsw::capi;
    DevBuf& pos = ctx->text_ws[TW_POS];
    uint64_t want_pos = std::max<uint64_t>(ix->n_bytes / pos_per_bytes + 64, pos.cap / 8);
    for (int round = 0; round < 2; ++round) {
        ZSW_HIP(ctx, pos.ensure(want_pos * 8));
        ix->pos = pos.as<uint64_t>();
        ix->pos_cap = want_pos;
        size_t tiles_tmp = 0;
        void* scan_tmp = nullptr;
        ZSW_HIP(ctx, index_scan_bytes(*ix, &tiles_tmp, stream));
        zsw_error err = size(tiles_tmp, &scan_tmp);
        if (err != ZSW_OK) return err;
        hipLaunchKernelGGL(state_init_kernel<WORDS>, dim3(1), dim3(1), 0, stream, d_state);
        ZSW_HIP(ctx, index_launch(ctx, *ix, round == 0, scan_tmp, tiles_tmp, stream, byte));
        err = launch(scan_tmp);
        if (err != ZSW_OK) return err;
        ZSW_HIP(ctx, hipMemcpyAsync(state, d_state, WORDS * 8, hipMemcpyDeviceToHost, stream));
        ZSW_HIP(ctx, hipStreamSynchronize(stream));
        if (!state[ST_OVERFLOW]) return ZSW_OK;
        if (round == 1) break;
        want_pos = state[ST_NEWLINES] + 64;
    }
    return fail(ctx, ZSW_ERR_HIP, twice);
}

}  // namespace text
}  // namespace zsw
