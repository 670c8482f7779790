// zsw_strand.hpp — the strand-aware calls (zsw_strand.hip): what the seed kernel stores per read, the complement table and the
// slots of the context's strand workspace. Not installed.
#pragma once
#include <stdint.h>

namespace zsw {

// read byte -> byte of the complementary base
struct ComplementTable {
    uint8_t t[256];
};

// The default: the IUPAC nucleotide complement, case preserved, every other byte mapped to itself.
inline void complement_default(uint8_t* t) {
    for (int b = 0; b < 256; ++b) t[b] = (uint8_t)b;
    const char* from = "ACGTURYSWKMBDHVN";
    const char* to = "TGCAAYRSWMKVHDBN";
    for (int k = 0; from[k]; ++k) {
        t[(uint8_t)from[k]] = (uint8_t)to[k];
        t[(uint8_t)(from[k] | 0x20)] = (uint8_t)(to[k] | 0x20);
    }
}

// 8 bytes per read: x = claim W's bound of the forward strand | of the reverse strand << 16 (seed_bound_u16: 0xffff = none),
// y = support of the anchor vote forward | reverse << 8 | the strand that runs first << 16
__host__ __device__ inline uint2 strand_meta_pack(uint32_t u_f, uint32_t u_r, int sup_f, int sup_r, int first) {
    return make_uint2(u_f | (u_r << 16), (uint32_t)sup_f | ((uint32_t)sup_r << 8) | ((uint32_t)first << 16));
}
__host__ __device__ inline uint32_t strand_meta_first(uint2 m) { return (m.y >> 16) & 1u; }
__host__ __device__ inline uint32_t strand_meta_bound(uint2 m, int strand) { return strand ? m.x >> 16 : m.x & 0xffffu; }

constexpr int STRAND_RECORD_INTS = 8;  // zsw_debug_strand_records

// zsw_context::st_ws
enum { ST_IN = 0, ST_IN_OFF, ST_ORIENT, ST_META, ST_LIST, ST_COUNTS, ST_SECOND, ST_SECOND_OFF, ST_SCAN_TMP, ST_S2_SCORE, ST_S2_STATUS,
       ST_S2_TIER, ST_OUT_SCORE, ST_OUT_STATUS, ST_OUT_TIER, ST_OUT_STRAND, ST_ORIENT_FINAL };
// ST_COUNTS (uint32): settled forward, settled reverse, scored on both strands (the length of ST_LIST), answered as reverse
enum { STC_SETTLED_F = 0, STC_SETTLED_R, STC_BOTH, STC_REVERSE, STC_N };

}  // namespace zsw
