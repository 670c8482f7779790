// zsw_panel.hpp — reference panels (zsw_panel.hip): the members the context keeps, what the seed kernel reads per member and
// stores per read, the layout of zsw_debug_panel_records and the slots of the panel workspace. Not installed.
#pragma once
#include <stdint.h>

#include <vector>

#include "zsw_context.hpp"

namespace zsw {

constexpr uint32_t PANEL_MAX_REFS = 64;  // ZSW_PANEL_MAX_REFS: one bit per member in a read's 64-bit list of members still to score

// What panel_seed_kernel reads per member, from device memory (64 of them do not fit kernel arguments)
struct PanelMemberDev {
    SeedParams sp;
    const uint2* table;  // the member's index; null: no usable index, the member has no bound and no support
    uint32_t same_sweep; // 1: sp equals the previous member's, the sweep of the read is reused
    uint32_t pad;
};

// zsw_debug_panel_records, 2 + 2 * n_refs int32 per read: the first-choice member, 1 = settled after one score, the n_refs
// supports of the anchor vote, the n_refs whole-reference bounds (-1: none)
inline size_t panel_record_ints(uint32_t n_refs) { return 2 + 2 * (size_t)n_refs; }

struct PanelMember {
    uint64_t start = 0;  // of the member in Panel::d_seqs / h_seqs
    uint64_t len = 0;
    SeedIndex index;     // built with the first panel call that can use it, rebuilt after zsw_set_scoring
};

// Panel::ws
enum { PW_IN = 0, PW_IN_OFF, PW_MEMBERS, PW_FIRST, PW_BOUNDS, PW_TODO, PW_COUNTS, PW_LIST, PW_NSEL, PW_SEL_TMP, PW_GROUP, PW_GROUP_OFF, PW_SCAN_TMP,
       PW_G_SCORE, PW_G_STATUS, PW_G_TIER, PW_OUT_SCORE, PW_OUT_STATUS, PW_OUT_TIER, PW_OUT_REF, PW_GA_IN, PW_GA_IN_OFF, PW_GA_REF, PW_N };
// PW_COUNTS (uint32): reads settled after one score, reads scored against every member, then the sizes of the first round's groups
// and of the second round's lists, one per member each
enum { PC_SETTLED = 0, PC_ALL, PC_ROUND1, PC_ROUND2 = PC_ROUND1 + PANEL_MAX_REFS, PC_N = PC_ROUND2 + PANEL_MAX_REFS };

struct Panel {
    std::vector<PanelMember> members;
    DevBuf d_seqs;                // every member at a 256-byte boundary, 16 bytes of slack behind each
    std::vector<uint8_t> h_seqs;  // the same layout on the host: the indices are built from it
    std::vector<PanelMemberDev> h_members;  // what the last call sent to ws[PW_MEMBERS]
    DevBuf ws[PW_N];
    uint64_t counts[4] = {0, 0, 0, 0};  // zsw_panel_counts of the last call
};

}  // namespace zsw
