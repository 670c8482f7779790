// zsw_align.hpp — entry points of the alignment (traceback) kernels (zsw_align.hip).
#pragma once
#include "zsw_internal.hpp"

namespace zsw {

// Pass 2 for one <N lanes, nv vectors> group of reads (b.items lists them).
hipError_t align_pass2(int N, uint32_t nv, const BatchDev& b, const uint8_t* d_ref, uint32_t ref_len, const ScoringDev* d_sc,
                       int S, const uint32_t* d_score, const uint32_t* d_ref_end, const uint8_t* d_status, uint32_t W,
                       uint32_t maxc, uint8_t* d_ring, uint32_t grid, uint32_t* d_cig, uint64_t pool_base, int by_item,
                       uint64_t* d_cig_start, uint32_t* d_cig_raw, zsw_alignment* d_aln, uint32_t* d_fb_list,
                       uint32_t* d_fb_count, int invert, hipStream_t stream, const uint32_t* d_safe_row = nullptr);
size_t align_ring_bytes(int N, uint32_t nv, uint32_t W, uint32_t grid);
size_t align_lds_need(uint32_t nv, int S);
// count_only: per-block sums + total of n_ciglets; otherwise the packed write (and range inversion).
hipError_t align_finalize(zsw_alignment* d_aln, const uint8_t* d_status, uint32_t n, uint64_t* d_block_sums,
                          uint64_t* d_total, const uint64_t* d_cig_start, const uint32_t* d_cig_raw, int invert,
                          uint32_t* out_inc, uint8_t* out_op, uint64_t cap, bool count_only, hipStream_t stream);

// The packed kernel (zsw_align_pk_kernel.hpp): two reads per lane group in 16-bit halves. It takes groups of 8..64 lanes and
// up to 32 vectors whose striped profile fits LDS, and reads whose score stays below 2^15 with head-room (signed packed max).
constexpr uint32_t ALIGN_PK_MAX_SCORE = 30000;
bool align_pk_supported(int N, uint32_t nv, int S);
uint32_t align_pk_grid(int N, uint32_t nv, int S, uint32_t count, uint32_t cu_count);  // blocks that fill the chip once
size_t align_pk_ring_bytes(int N, uint32_t nv, uint32_t W, uint32_t grid);
hipError_t align_pass2_pk(int N, uint32_t nv, const BatchDev& b, const uint8_t* d_ref, uint32_t ref_len, const ScoringDev* d_sc,
                          int S, const uint32_t* d_score, const uint32_t* d_ref_end, const uint8_t* d_status, uint32_t W,
                          uint32_t maxc, uint8_t* d_ring, uint32_t grid, uint32_t* d_cig, uint64_t pool_base, int by_item,
                          uint64_t* d_cig_start, uint32_t* d_cig_raw, zsw_alignment* d_aln, uint32_t* d_fb_list,
                          uint32_t* d_fb_count, int invert, hipStream_t stream, const uint32_t* d_safe_row = nullptr);

// Device-side grouping (zsw_group.hip): read ids sorted by (N, packed/wide, nv, ref_end) + the table of group starts.
size_t group_temp_bytes(uint32_t n);
hipError_t group_reads(const BatchDev& b, const uint8_t* d_status, const uint8_t* d_tier, const uint32_t* d_ref_end, const uint32_t* d_score,
                       const uint32_t* d_safe_row /* may be null */, int lanes_w8, int lanes_w16, int lanes_w32, uint64_t* keys_in, uint64_t* keys_out, uint32_t* vals_in, uint32_t* items_out,
                       void* temp, size_t temp_bytes, uint32_t* table, uint32_t* table_count, uint32_t cap, hipStream_t stream);

// Third pass of sw_align_3pass (zsw_threepass.hip). list == null: classify pass over all reads (resolves the no-gaps
// shortcut, queues the rest in dp_list); otherwise the DP pass over `list`.
// The resources of its launches (threepass_third_pass, zsw_capi.hip; tests/test_gpu_threepass_edges.py reads these lines):
constexpr uint64_t THREEPASS_SLOT_CAP = 98304;             // bytes: the most a slot of the first DP launch holds (96 KiB)
constexpr uint32_t THREEPASS_MAXC = 32;                    // ciglets per read of the classify and first DP launches
constexpr uint64_t THREEPASS_SCRATCH_BUDGET = 2147483648;  // bytes of slot scratch a DP launch may ask for (2 GiB)
constexpr uint32_t THREEPASS_MAX_SLOTS = 131072;           // slots of a DP launch at most (at least 64: one block)
constexpr int THREEPASS_RECORD_INTS = 8;                   // zsw_debug_threepass_records
struct ThreePassArgs {
    BatchDev b{};
    const uint8_t* ref = nullptr;
    uint32_t ref_len = 0;
    const ScoringDev* sc = nullptr;
    const uint32_t* score = nullptr;  // ranges results, indexed by read id
    const uint32_t *rs = nullptr, *re = nullptr, *qs = nullptr, *qe = nullptr;
    const uint8_t* status = nullptr;
    const uint32_t* list = nullptr;  // read ids that need the DP (class 2), or null: classify pass over all reads
    const uint32_t* list_count = nullptr;
    uint32_t* dp_list = nullptr;     // classify pass: reads that need the DP
    uint32_t* dp_count = nullptr;
    uint32_t* dp_need_max = nullptr;  // classify pass: largest slot need (bytes) among them
    uint8_t* scratch = nullptr;       // DP pass: slots * slot_bytes
    uint32_t slots = 0;
    uint64_t slot_bytes = 0;
    uint32_t* cig = nullptr;          // ciglet pool (traceback order), maxc per read
    uint32_t maxc = 0;
    uint64_t pool_base = 0;
    int by_item = 0;
    uint64_t* cig_start = nullptr;
    uint32_t* cig_raw = nullptr;
    zsw_alignment* aln = nullptr;
    uint32_t* fb_list = nullptr;      // ciglet overflow / slot too small -> rerun with larger resources
    uint32_t* fb_count = nullptr;
    int invert = 0;
    // The shared-profile role (profile_set.rs:552-560: one profile, built from `pseq`, reused for every sequence of the batch):
    // non-null = the roles of three_pass.rs:21-26 are `reference` = read i, `query` = pseq for every i (ranges from
    // zsw_score_ranges_shared_batch: rs/re index the read, qs/qe the profile sequence); `ref` / `ref_len` are then unused.
    const uint8_t* pseq = nullptr;
    uint32_t pseq_len = 0;
    // Certificate mode of the classify pass (sw_simd_align's second pass skipped, zsw_capi.hip run_align; the decision is
    // zsw_cert.hpp's cert_decide, with the host models tests/models/align_gapless_cert.cpp and align_onegap_cert.cpp):
    // cert_ok[i] = both maxima of read i sit in one cell each (forward and reversed seeded pass, mode 3). A read whose only optimal
    // alignment is the gapless diagonal or has one gap run gets it here (cert_done[i] = 1), which is what sw_simd_align returns at
    // every <T, N>; every other read is left to the literal striped kernel (cert_done[i] = 0).
    const uint8_t* cert_ok = nullptr;
    uint8_t* cert_done = nullptr;
    int cert_maxw = 0, cert_go = 0, cert_ge = 0;
    int32_t* cert_rec = nullptr;  // zsw_debug_cert_records: CERT_RECORD_INTS per read (verdict, parameter, ties, sweep launch)
    // The sweeps over the two-run alternatives cost a read several times the rest of the certificate, and one read in seven needs
    // them: with one thread per read the other lanes of its wavefront would wait. The classify launch therefore lists those reads
    // (sweep_list / sweep_count) and a second launch — list = that list, sweep_pass = true: classify code, sweeps included — takes
    // them, every lane busy.
    uint32_t* sweep_list = nullptr;
    uint32_t* sweep_count = nullptr;
    bool sweep_pass = false;
    // zsw_debug_threepass_records: THREEPASS_RECORD_INTS per read (route, accepted band, attempts, launch, why the first DP launch
    // handed the read to the rerun, the band that did not fit, slot bytes, ciglets); tp_launch: 0 classify, 1 first DP launch, 2 rerun
    int32_t* tp_rec = nullptr;
    int tp_launch = 0;
};

hipError_t launch_threepass(const ThreePassArgs& a, uint32_t grid, hipStream_t stream);

}  // namespace zsw
