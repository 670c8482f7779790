// zsw_seed_diag_body.inc — the body of seed_diag_kernel (zsw_score_band.hip, which describes it), included as text by that kernel and
// by seed_diag_handback_kernel, so that the former compiles to what it was. In scope where it is included: the template arguments
// D, UNI and MINS, and `a` (SeedBandArgs). It uses no blockIdx: its work comes from the queue at a.next_pair.
    constexpr int TAG = -1;
    static_assert(D == 16, "a group of columns is two dwords of residue codes and 16 bits per read in the column masks");
    static_assert(D <= SEED_GROUP_MAX, "three k-mers per group (zsw_seed_diag.hpp)");
    static_assert(SEED_NARROW_WU_PER16 == 0 && SEED_NARROW_WD_PER32 == 0, "the window's height is fixed at compile time");
    __shared__ uint16_t sel_lut[16];
    __shared__ int sst[UNI ? 1 : BF_N * BLOCK];  // (the layout fields only: the programmes' state lives in registers)
    const int tid = threadIdx.x;
    int* const st = sst + (UNI ? 0 : tid);
    if (tid < 16) {
        const uint32_t k = (uint32_t)tid;
        sel_lut[tid] = (uint16_t)(k < 4 ? (2 * k + 1) | ((8 + k) << 8) : (k == 15 ? 0x0c00u : (2 * (k - 3)) | 0x0c00u));
    }
    __syncthreads();
    const int R = (int)a.ref_len;
    const uint32_t n_items = a.n_dev ? min(*a.n_dev, a.n) : a.n;
    const uint32_t n_pairs = (n_items + 1) / 2;
    const bool bail = a.bail_check && a.accepted && ((uint64_t)(*a.accepted) * SEED_BAIL_RATIO < (uint64_t)n_items || n_items < a.bail_below);
    uint32_t n_accepted = 0;
    uint32_t n_below = 0;  // (MINS)
    const uint32_t ge2 = a.ge2, gd2 = a.gd2;
    const uint32_t ge1 = ge2 & 0xffffu;
    const uint32_t maxw2 = (uint32_t)a.sp.maxw * 0x00010001u, go2p = (uint32_t)a.sp.go * 0x00010001u;
    const int wu = a.wu0, wd = a.wd0;  // (launch_seed_band: wu + wd + 1 + SEED_DIAG_SLACK == D)
    // UNI: the one layout of the launch
    int um = 0, ustride = 0, uc0 = 0;
    uint32_t umagic = 0, ulam2 = 0;
    if (UNI) {
        seed_layout((int)a.b.fixed_len, a.sp.K, a.sp.spacer, &um, &ustride, &uc0);
        umagic = seed_div_magic(ustride);
        ulam2 = (uint32_t)seed_lambda(a.sp, ustride) * 0x00010001u;
    }
    // the per-row table by byte offset from row 0: the rows outside the reference, above it or below, share the neutral entry of row R
    const char* const gt = reinterpret_cast<const char*>(a.gtab + SEED_GTAB_PAD);
    const uint32_t row_end = (uint32_t)R * (uint32_t)sizeof(uint2);

    for (;;) {
        BandPair P;
        const int fetched = band_fetch(a, tid, n_items, n_pairs, bail, SEED_DIAG_SLACK, &P);
        if (fetched == 0) break;
        if (fetched == 2) {
        const uint32_t ridA = P.ridA, ridB = P.ridB;
        const bool validB = P.validB;
        const int lenA = UNI ? (int)a.b.fixed_len : (int)P.lenA, lenB = UNI ? (validB ? (int)a.b.fixed_len : 0) : (int)P.lenB;
        const int lenmax = UNI ? (int)a.b.fixed_len : max(lenA, lenB);
        const int dtmin = min(P.dtA, P.dtB), dtmax = max(P.dtA, P.dtB);
        // the band's last diagonal: D - 1 for a pair with two anchors, D - 2 otherwise (then diagonal D - 1 stands for the cells
        // below the band: it hands yf to the band's last cell, and its own value counts for nothing)
        const bool narrow = dtmax - dtmin < SEED_DIAG_SLACK;
        const uint32_t infoA = a.info[ridA], infoB = a.info[ridB];
        // the k-mer masks of the pair, read A's 16 bits below read B's (a missing partner has none): above the band fa, below it fb
        const uint32_t masksA = a.band_masks[ridA], masksB = validB ? a.band_masks[ridB] : 0u;
        const uint32_t fa2 = __builtin_amdgcn_perm(masksB, masksA, 0x05040100u), fb2 = __builtin_amdgcn_perm(masksB, masksA, 0x07060302u);
        uint32_t lam2 = ulam2;
        if (!UNI) {
            band_lane_init(a.sp, st, lenA, masksA, lenB, masksB);
            lam2 = (uint32_t)st[BF_LAM2 * BLOCK];
        }
        const uint32_t lamx = pk_subu_sat(lam2, maxw2);
        const uint32_t* codeA = a.codes + (size_t)ridA * a.cs;
        const uint32_t* codeB = a.codes + (size_t)ridB * a.cs;
        const int base = dtmin - wu;  // diagonal j crosses row base + c + j in column c
        const auto table_row = [&](uint32_t off) { return *reinterpret_cast<const uint2*>(gt + min(off, row_end)); };  // off: 8 * row, as it wraps
        uint2 w[D];                   // slot (c + j) % D: the table entry of the row diagonal j crosses in column c
        uint32_t H[D], F[D];          // H of the previous column (drift of that column), outgoing F (drift of this one)
        uint32_t Dc = (a.floor0 - ge1) * 0x00010001u;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            w[j] = table_row((uint32_t)(base + j) * (uint32_t)sizeof(uint2));
            H[j] = Dc;
            F[j] = pk_addu(Dc, ge2);
        }
        uint32_t Fbelow = pk_addu(Dc, ge2);  // what the cell below the band's last sends right
        BandPk up, lo;
        up.ch = lo.ch = PKB2;
        up.fr = lo.fr = 0;
        uint32_t oa2 = 0, ob2 = 0, best = 0;
        // One wave-uniform choice (UNI; ZSW_DEBUG_SEED_DIAG_MASKED switches it off), taken once per wavefront and walk: the INTERIOR copy
        // of the column loop, if every active lane's pair is `narrow` and its walk stays inside the reference (diag_walk_is_interior:
        // the edge words above, topin, below, exits and yfok are all-ones in every executed column). A one-length batch has realA
        // all-ones in those columns too, so the six masks built from them (inj, join, ex, bel, nm through pair_mask, topin through
        // lane_mask) are all-ones wherever they matter and the copy passes their operands unmasked. With every pair narrow, diagonal
        // D - 1 counts for nothing in the whole wavefront: the copy does not compute its cell (H[D - 1] goes stale, nothing reads it;
        // F[D - 1] = Fbelow as ever). Two cases differ from the masked loop, and neither reaches a result:
        // (a) a lane without a partner (lenB == 0) has realB == 0, so the masked loop clears the high half of every masked operand.
        //     Unmasked, that half walks the neutral codes of the missing read and holds values the masked loop would not.
        //     band_finish never reads the high half of such a lane, and the low half cannot see it: the packed instructions keep the
        //     halves apart, and in the plain 32-bit additions, subtractions and left shifts (up.ch += maxw2, h - gd2, ... - ge2,
        //     pk_tag's v << 1) a carry, a borrow or a shifted bit travels from the low half to the high one only.
        // (b) join is 0 in a read's last column: the first cell of that column joins nothing. What it would feed, up.fr / up.ch, is
        //     read by the next column's v alone, and a one-length batch has no column behind lenmax - 1.
        // tests/test_gpu_diag_interior.py compares both with the masked loop, record for record.
        const bool interior = UNI && !a.diag_masked && __ballot(!(narrow && diag_walk_is_interior(dtmin, dtmax, wu, wd, lenmax, R))) == 0;
        const auto walk = [&](auto interior_copy) __attribute__((always_inline)) {
        constexpr bool INTERIOR = decltype(interior_copy)::value;
#pragma unroll 1
        for (int k0 = 0; k0 < lenmax; k0 += D) {
            // the group's residue codes; a column's selectors are looked up one column ahead of their use (sixteen selectors held
            // across the group would be twelve registers more than the two copies of the loop leave free)
            uint32_t wa[D / 8], wb[D / 8];
#pragma unroll
            for (int d = 0; d < D / 8; ++d) {
                const uint32_t di = (uint32_t)(k0 / 8 + d);
                wa[d] = di < a.cs ? codeA[di] : 0xffffffffu;
                wb[d] = (validB && di < a.cs) ? codeB[di] : 0xffffffffu;
            }
            const auto sel_of = [&](int c) __attribute__((always_inline)) {
                return (uint32_t)sel_lut[(wa[c / 8] >> (4 * (c % 8))) & 15u] | ((uint32_t)sel_lut[(wb[c / 8] >> (4 * (c % 8))) & 15u] << 16);
            };
            uint32_t sel_next = sel_of(0);
            // the group's columns as bit masks: the k-mer events of both programmes, and where the band's ends are cells of the matrix
            uint32_t upS, upE, loS, loE, loI, freeb, anyup, anylo, inj = 0, join = 0, ex = 0, bel = 0, nm = 0, topin = 0;
            uint32_t gany = 0xffffu;  // UNI: the columns in which a k-mer of the layout starts or ends, on scalar registers
            {
                DiagGroupEvents ev;
                if (UNI) {  // (a missing partner shares A's patterns: its masks are 0)
                    const SeedGroupPatterns g = seed_group_patterns(k0, D, um, uc0, ustride, a.sp.K, a.sp.spacer, umagic);
                    ev = diag_group_events(g, g, fa2, fb2);
                    gany = g.start[0] | g.start[1] | g.start[2] | g.end[0] | g.end[1] | g.end[2];
                } else {
                    const BandLayout yA = band_layout(st, false), yB = band_layout(st, true);
                    ev = diag_group_events(seed_group_patterns(k0, D, yA.m, yA.c0, yA.stride, a.sp.K, a.sp.spacer, yA.magic),
                                           seed_group_patterns(k0, D, yB.m, yB.c0, yB.stride, a.sp.K, a.sp.spacer, yB.magic), fa2, fb2);
                }
                upS = ev.upS;
                upE = ev.upE;
                loS = ev.loS;
                loE = ev.loE;
                loI = ev.loI;
                freeb = ev.freeb;
                anyup = upS | upE;
                anyup |= anyup >> 16;
                anylo = loS | loE;
                anylo |= anylo >> 16;
                if (!INTERIOR) {
                // column c: first row base + c (a cell above it exists if that is > 0), first row below dtmax + c + 1 + wd
                const int t0 = base + k0, t1 = dtmax + k0 + 1 + wd;
                const uint32_t above = seed_bits_from(1 - t0), below = seed_bits_below(R - t1);
                topin = seed_bits_from(-t0) & seed_bits_below(R - t0);                                   // the first row is a row of the reference
                const uint32_t exits = below & seed_bits_from(1 - t1), yfok = below & seed_bits_from(-t1);  // ... the last row; the next column's last row
                const uint32_t realA = seed_bits_below(lenA - k0), realB = seed_bits_below(lenB - k0);
                inj = pair_bits(realA & above, realB & above);
                join = pair_bits(seed_bits_below(lenA - k0 - 1) & topin, seed_bits_below(lenB - k0 - 1) & topin);  // (not behind the read's last column)
                ex = pair_bits(realA & exits, realB & exits);
                bel = pair_bits(realA & below, realB & below);
                nm = pair_bits(realA & yfok, realB & yfok);
                }
            }
            const uint32_t enter = (uint32_t)(base + k0 + D) * (uint32_t)sizeof(uint2);  // column k0's entering row, as a byte offset
#pragma unroll
            for (int u = 0; u < D; ++u) {
                if (k0 + u < lenmax) {  // (no break: a loop with two exits around a __ballot is not unrolled)
                const uint32_t sel_u = sel_next;
                if (u + 1 < D) sel_next = sel_of(u + 1);
                Dc = pk_addu(Dc, ge2);
                const uint32_t Dn = pk_addu(Dc, ge2);
                // above the column: a(c); the band's first cell receives it from above (E: less gap_open)
                up.ch += maxw2;
                up.fr += maxw2;
                // (UNI: no lane has an event in a column where the layout has none; the scalar test spares the vector one)
                if ((!UNI || ((gany >> u) & 1u) != 0) && __ballot((anyup >> u) & 1u) != 0) pk_events(&up, pair_mask(upS, u), pair_mask(upE, u), lam2);
                uint32_t v = pk_subu_sat(pk_maxu(up.ch, up.fr), PKB2);
                if (!INTERIOR) v &= pair_mask(inj, u);
                oa2 = pk_maxu(oa2, v);
                uint32_t vin = pk_subu_sat(v, go2p);
                if (!INTERIOR) vin &= lane_mask(topin, u);
                uint32_t E = pk_addu(Dc, pk_tag<TAG>(vin));
                uint32_t rmax = 0x04000400u;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (j == D - 1 && INTERIOR) {
                        rmax = pk_maxu(rmax, H[j - 1]);
                        break;
                    }
                    const uint2 wr = w[(u + j) % D];
                    const uint32_t hd = pk_addu(H[j], __builtin_amdgcn_perm(wr.y, wr.x, sel_u));
                    const uint32_t Fin = j + 1 < D ? F[j + 1 < D ? j + 1 : j] : Fbelow;
                    const uint32_t h = pk_max3(hd, E, Fin);
                    H[j] = h;
                    const uint32_t hg = h - gd2;
                    F[j] = pk_max3(Fin, hg, Dn);
                    E = pk_max3(E, hg, Dn) - ge2;
                    if (j == D - 1) rmax = pk_max3(rmax, H[j - 1], narrow ? 0u : h);
                    else if (j & 1) rmax = pk_max3(rmax, H[j - 1], h);
                    if (j == 0) w[u] = table_row(enter + (uint32_t)u * (uint32_t)sizeof(uint2));  // the row that enters the window in the next column
                }
                best = pk_maxu(best, pk_subu(rmax, Dc));
                // the first cell's value joins the paths above the band behind this column
                {
                    uint32_t ux = pk_addu(pk_untag<TAG>(pk_subu(H[0], Dc)), PKB2);
                    if (!INTERIOR) ux &= pair_mask(join, u);
                    const uint32_t fm = pair_mask(freeb, u);
                    up.fr = pk_maxu(up.fr, ux & fm);
                    up.ch = pk_maxu(up.ch, ux & ~fm);
                }
                // below the column: b(c), joined by the band's last cell
                lo.ch += maxw2;
                lo.fr += maxw2;
                if ((!UNI || ((gany >> u) & 1u) != 0) && __ballot((anylo >> u) & 1u) != 0) pk_events(&lo, pair_mask(loS, u), pair_mask(loE, u), lam2);
                uint32_t he = pk_addu(pk_untag<TAG>(pk_subu((INTERIOR || narrow) ? H[D - 2] : H[D - 1], Dc)), PKB2);
                if (!INTERIOR) he &= pair_mask(ex, u);
                const uint32_t im = pair_mask(loI, u);
                lo.fr = pk_maxu(lo.fr, he & im);
                lo.ch = pk_maxu(lo.ch, he & ~im);
                const uint32_t b2 = pk_subu_sat(pk_maxu(lo.ch, lo.fr), PKB2);
                ob2 = pk_maxu(ob2, INTERIOR ? b2 : b2 & pair_mask(bel, u));
                // the next column's last cell: F entering from the left (the bound may have stood lambda - maxw higher just before a
                // k-mer's last column; a horizontal run opens with gap_open)
                uint32_t yf = pk_subu_sat(pk_addu(b2, lamx), go2p);
                if (!INTERIOR) yf &= pair_mask(nm, u);
                Fbelow = pk_addu(Dn, pk_tag<TAG>(yf));
                if (INTERIOR || narrow) F[D - 1] = Fbelow;
                }
            }
        }
        };  // walk
        if constexpr (UNI) {
            if (interior) walk(std::true_type{});
            else walk(std::false_type{});
        } else {
            walk(std::false_type{});
        }
        band_finish<0, MINS>(a, P, best, oa2, ob2, dtmin, dtmax, lenmax | (wu << 8) | (wd << 20), 1, infoA, infoB, BandEnds{}, &n_accepted, &n_below);
        }  // fetched == 2
    }
    band_count_accepted(a, tid, n_accepted);
    if (MINS) band_count_below(a, tid, n_below);
