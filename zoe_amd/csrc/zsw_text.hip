// zsw_text.hip — the newline index of zsw_fastq_parse_batch and zsw_sam_parse_batch, and the same index over '>' for
// zsw_fasta_parse_batch (declared in zsw_text_dev.hpp; the rules are
// zsw_text.hpp, shared with the host models):
//   count     newlines per tile of FQ_TILE bytes: 16-byte loads, the head and the tail granule peeled byte by byte
//   scan      hipcub's exclusive sum over the tile counts; its last entry is the number of newlines
//   positions the same sweep again: the position of every newline at its rank (a prefix across the lanes plus the tile's base)
// and index_prepare, which stages the text of a host call and sizes the tile arrays. The buffers are zsw_context::text_ws.
#include "zsw_text_dev.hpp"

using namespace zsw;
using namespace zsw::capi;

namespace zsw {
namespace text {
namespace {

constexpr uint32_t TILE_BLOCK = FQ_G * FQ_TILE_WAVES;

// the wavefront behind granule_words and put_newlines
struct TileIo {
    const uint8_t* text;
    uint64_t* pos_out;

    __device__ __forceinline__ uint8_t byte(uint64_t p) const { return text[p]; }
    __device__ __forceinline__ void load16(uint64_t p, uint32_t w[4]) const {
        const u32x4 v = *reinterpret_cast<const u32x4_alias*>(text + p);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    __device__ __forceinline__ void put_position(uint64_t rank, uint64_t p) const { pos_out[rank] = p; }
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 1; d < FQ_G; d <<= 1) x += __shfl_xor(x, d, FQ_G);
    return x;
}

// POSITIONS = false: tile_counts[t] = the newlines of tile t. POSITIONS = true: pos[rank] for every newline. BYTE: what counts as one.
template <bool POSITIONS, uint8_t BYTE>
__global__ __launch_bounds__(TILE_BLOCK) void newline_kernel(IndexArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * FQ_TILE_WAVES + (threadIdx.x >> 6);
    const uint64_t stride = (uint64_t)gridDim.x * FQ_TILE_WAVES;
    if (!POSITIONS && blockIdx.x == 0 && threadIdx.x == 0) a.tile_counts[a.n_tiles] = 0;  // the exclusive sum's last input: its output is the total
    TileIo io{a.text, a.pos};
    for (uint64_t t = wave; t < a.n_tiles; t += stride) {
        uint32_t w[FQ_TILE_SWEEPS][4];
#pragma unroll
        for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) granule_words(io, a.head, a.n_bytes, (t * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane, w[s]);
        if (!POSITIONS) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) c += words_newlines<BYTE>(w[s]);
            c = wave_sum(c);
            if (lane == 0) a.tile_counts[t] = c;
        } else {
            uint64_t base = uni(a.tile_base[t]);
#pragma unroll
            for (uint32_t s = 0; s < FQ_TILE_SWEEPS; ++s) {
                const uint32_t c = words_newlines<BYTE>(w[s]);
                const uint32_t x = lane_prefix_sum(c, lane);
                if (c) put_newlines<BYTE>(io, w[s], a.head, (t * FQ_TILE_SWEEPS + s) * FQ_G + (uint32_t)lane, base + (x - c), a.pos_cap);
                base += uni((uint32_t)__shfl(x, FQ_G - 1, FQ_G));
            }
        }
    }
}

}  // namespace

uint32_t grid_for(const zsw_context* ctx, uint64_t items, uint32_t per_block) {
    const uint64_t want = (items + per_block - 1) / per_block;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->cu_count * 8u));
}

zsw_error index_prepare(zsw_context* ctx, IndexArgs* ix, const uint8_t* text, uint64_t n_bytes, bool host, hipStream_t stream) {
    DevBuf* ws = ctx->text_ws;
    static_assert(TW_N <= sizeof(ctx->text_ws) / sizeof(ctx->text_ws[0]), "zsw_context::text_ws holds every buffer");
    ix->text = text;
    ix->n_bytes = n_bytes;
    if (host) {  // the text crosses once
        ZSW_HIP(ctx, ws[TW_TEXT].ensure(n_bytes + 16));
        if (n_bytes) ZSW_HIP(ctx, hipMemcpyAsync(ws[TW_TEXT].p, text, n_bytes, hipMemcpyHostToDevice, stream));
        ix->text = ws[TW_TEXT].as<uint8_t>();
    }
    ix->head = (uint32_t)(reinterpret_cast<uintptr_t>(ix->text) & 15u);
    ix->n_tiles = tiles_of(ix->head, n_bytes);
    ZSW_HIP(ctx, ws[TW_TILE_COUNTS].ensure((ix->n_tiles + 1) * 8));
    ZSW_HIP(ctx, ws[TW_TILE_BASE].ensure((ix->n_tiles + 1) * 8));
    ix->tile_counts = ws[TW_TILE_COUNTS].as<uint64_t>();
    ix->tile_base = ws[TW_TILE_BASE].as<uint64_t>();
    return ZSW_OK;
}

hipError_t index_scan_bytes(const IndexArgs& ix, size_t* bytes, hipStream_t stream) {
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, ix.tile_counts, const_cast<uint64_t*>(ix.tile_base), (int)(ix.n_tiles + 1), stream);
}

template <uint8_t BYTE>
hipError_t index_launch_of(const zsw_context* ctx, const IndexArgs& ix, bool count, void* scan_tmp, size_t scan_bytes, hipStream_t stream) {
    if (!ix.n_tiles) return hipSuccess;
    const uint32_t tile_grid = grid_for(ctx, ix.n_tiles, FQ_TILE_WAVES);
    if (count) {
        hipLaunchKernelGGL((newline_kernel<false, BYTE>), dim3(tile_grid), dim3(TILE_BLOCK), 0, stream, ix);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, ix.tile_counts, const_cast<uint64_t*>(ix.tile_base), (int)(ix.n_tiles + 1), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((newline_kernel<true, BYTE>), dim3(tile_grid), dim3(TILE_BLOCK), 0, stream, ix);
    return hipGetLastError();
}

hipError_t index_launch(const zsw_context* ctx, const IndexArgs& ix, bool count, void* scan_tmp, size_t scan_bytes, hipStream_t stream, uint8_t byte) {
    return byte == '>' ? index_launch_of<'>'>(ctx, ix, count, scan_tmp, scan_bytes, stream) : index_launch_of<'\n'>(ctx, ix, count, scan_tmp, scan_bytes, stream);
}

}  // namespace text
}  // namespace zsw
