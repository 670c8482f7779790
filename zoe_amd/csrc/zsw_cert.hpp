// zsw_cert.hpp — decision logic of the alignment certificate (the classify pass of zsw_threepass.hip in certificate mode), shared
// with its host models (tests/models/align_gapless_cert.cpp and align_onegap_cert.cpp compile this header with g++ and check every
// certificate it issues against plain Gotoh and the oracle's literal sw_simd_align).
//
// sw_simd_align's CIGAR depends on the <T, N> striping only where several optimal alignments exist. Given, from the forward and the
// reversed seeded pass, that (1) the maximum S of the matrix sits in exactly one cell (re - 1, qe - 1) and (2) the maximum of the
// reversed matrix sits in exactly one cell, (rs, qs) turned round, every alignment that scores S runs from (rs, qs) to
// (re - 1, qe - 1). Let rlen = re - rs, qlen = qe - qs and maxw the largest weight of the matrix. Then:
//
//   gapless  rlen == qlen =: n, (3) the weights of the diagonal from (rs, qs) add up to S, and (4) no other path between the corners
//            reaches S: three or more gap runs have at most n - 1 pairs and pay 3 * gap_open (ruled out by S > maxw * (n - 1) -
//            3 * gap_open); two runs are an insertion and a deletion of the same length k, in either order, with the pairs between
//            them on the diagonal k away — for every k that the potential maxw * (n - k) - 2 * gap_open - 2 * (k - 1) * gap_extend
//            does not rule out, the best placement of the two runs is one sweep over prefix sums, and it must stay below S.
//   one gap  g = |rlen - qlen| >= 1, m = min(rlen, qlen) >= 2, gap_extend > 0. (3) The alignments with ONE run of g are p pairs on
//            the first diagonal, the run, m - p pairs on the second, p = 1 .. m - 1: one sweep. One p must reach S, or several
//            ADJACENT ones (the same alignment shifted along a homopolymer run or a short repeat), of which the walk from the end
//            takes the LAST. (4) Three or more runs: S > maxw * m - 3 * gap_open - max(g - 3, 0) * gap_extend. Two runs of signed
//            lengths ra and rlen - qlen - ra (a deletion counts +, an insertion -): every ra with |ra| <= amax is swept — the
//            potential bounds the total run length by X, and |ra| + |rlen - qlen - ra| >= 2 |ra| - g — and must stay below S.
//
// Sweeps cost a read several times the rest of the certificate: the classify launch defers (CERT_DEFERRED) every read that needs
// them to a second launch over the deferred reads alone, which decides them with defer = false.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ZSW_CERT_HD __host__ __device__ __forceinline__
#else
#define ZSW_CERT_HD inline
#endif

namespace zsw {

// Verdict classes, as zsw_debug_cert_records reports them (include/zoe_sw.h).
enum CertVerdict : int32_t {
    CERT_NOT_UNIQUE = 0,  // a maximum is not in one cell (or the ranges are empty): no certificate is attempted
    CERT_GAPLESS = 1,     // certified: the diagonal is the only optimal alignment
    CERT_ONE_GAP = 2,     // certified: one gap run at the last of the adjacent optimal placements
    CERT_DIAG_SUM = 3,    // rejected: equal lengths, but the diagonal does not add up to the score
    CERT_POTENTIAL = 4,   // rejected: the potential does not rule out three or more runs (one gap: or m < 2, or gap_extend == 0)
    CERT_TWO_RUNS = 5,    // rejected: an alignment with two runs reaches the score
    CERT_PLACEMENT = 6,   // rejected: no single or adjacent set of one-run placements reaches exactly the score
    CERT_DEFERRED = 7,    // classify launch: the read needs the sweeps, decided by the second launch
};
constexpr int CERT_RECORD_INTS = 4;  // verdict, parameter, ties, 1 = decided by the sweep launch

struct CertScheme {
    long long maxw, go, ge;  // largest weight of the matrix; gap_open, gap_extend as positive magnitudes
};

struct CertResult {
    int32_t verdict = CERT_NOT_UNIQUE;
    // CERT_GAPLESS: run lengths k swept; CERT_ONE_GAP / CERT_PLACEMENT: the last best placement p; CERT_TWO_RUNS: the first run's
    // signed length (gapless: +k deletion first, -k insertion first); CERT_DIAG_SUM: the diagonal's sum (clamped to int32)
    int32_t param = 0;
    int32_t ties = 0;  // one gap: placements that reach the best score
    bool deferred = false;
};

template <typename Wt>
ZSW_CERT_HD int cert_maxw(const Wt* w, int S) {  // largest weight of an S x S matrix
    int maxw = 0;
    for (int i = 0; i < S * S; ++i) maxw = maxw > (int)w[i] ? maxw : (int)w[i];
    return maxw;
}

// The gapless certificate's first condition; the kernel computes the diagonal's sum only when it holds.
ZSW_CERT_HD bool cert_gapless_potential(const CertScheme& c, uint32_t n, uint32_t score) {
    return (long long)score > c.maxw * ((long long)n - 1) - 3ll * c.go;
}

// Two runs of k between the corners of a gapless diagonal of n pairs: pairs 0 .. i-1 on the diagonal, run, pairs i .. j-1 on the
// diagonal k rows (dir 0) or k columns (dir 1) away, run, pairs j+k .. n-1 on the diagonal again: score - 2go - 2ge(k-1) + A(j) - B(i)
// with A(j) = Q(j) - P0(j+k), B(i) = Q(i) - P0(i), 1 <= i <= j <= n-k-1. True if one of them reaches the score.
template <typename W>
ZSW_CERT_HD bool cert_gapless_two_runs(const W& wt, uint32_t n, uint32_t k, int dir, const CertScheme& c) {
    int64_t qv = 0, p0j = 0, p0jk = 0, low = INT64_MAX, best_alt = INT64_MIN;
    for (uint32_t t = 0; t < k; ++t) p0jk += wt(t, t);
    for (uint32_t j = 1; j + k + 1 <= n; ++j) {
        qv += dir == 0 ? wt(j - 1 + k, j - 1) : wt(j - 1, j - 1 + k);
        p0j += wt(j - 1, j - 1);
        p0jk += wt(j + k - 1, j + k - 1);
        const int64_t bj = qv - p0j;
        low = bj < low ? bj : low;
        const int64_t v = qv - p0jk - low;
        best_alt = v > best_alt ? v : best_alt;
    }
    return best_alt != INT64_MIN && best_alt - 2ll * c.go - 2ll * c.ge * ((long long)k - 1) >= 0;
}

// Two runs of signed lengths ra and rb = rlen - qlen - ra between the corners: i pairs on the first diagonal, run ra, j - i pairs on
// the diagonal ra away, run rb, the rest on the last diagonal: P0(i) + Pa(j) - Pa(i) + Pz(M) - Pz(j) - cost, 1 <= i <= j <= M - 1.
// True if one of them reaches the score.
template <typename W>
ZSW_CERT_HD bool cert_one_gap_two_runs(const W& wt, long long ap, long long an, long long bp, long long bn, long long M, long long cost, long long S) {
    int64_t pzM = 0;
    for (long long t = 0; t < M; ++t) pzM += wt(t + ap + bp, t + an + bn);
    int64_t s0 = 0, sa = 0, sz = 0, low = INT64_MAX, best_alt = INT64_MIN;
    for (long long j = 1; j <= M - 1; ++j) {
        s0 += wt(j - 1, j - 1);
        sa += wt(j - 1 + ap, j - 1 + an);
        sz += wt(j - 1 + ap + bp, j - 1 + an + bn);
        const int64_t bj = sa - s0;
        low = bj < low ? bj : low;
        const int64_t v = sa - sz - low;
        best_alt = v > best_alt ? v : best_alt;
    }
    return pzM - cost + best_alt >= S;
}

// The certificate of one read. wt(i, j): weight of reference[rs + i] against query[qs + j]; diag_sum(): the sum of wt(t, t) over
// t < rlen (the kernel sums four residues per load); unique: both maxima sit in one cell each; defer: classify launch (reads that
// need the sweeps get CERT_DEFERRED).
template <typename W, typename D>
ZSW_CERT_HD CertResult cert_decide(const W& wt, const D& diag_sum, bool unique, uint32_t rs, uint32_t re, uint32_t qs, uint32_t qe,
                                   uint32_t score, const CertScheme& c, bool defer) {
    CertResult r;
    if (!(unique && re > rs && qe > qs)) return r;
    const uint32_t rlen = re - rs, qlen = qe - qs;
    const long long S_ = (long long)score;
    if (qlen == rlen) {
        if (!cert_gapless_potential(c, rlen, score)) {
            r.verdict = CERT_POTENTIAL;
            return r;
        }
        const int64_t sum = diag_sum();
        if ((sum < 0 ? 0u : (uint32_t)sum) != score) {
            r.verdict = CERT_DIAG_SUM;
            r.param = sum > INT32_MAX ? INT32_MAX : sum < INT32_MIN ? INT32_MIN : (int32_t)sum;
            return r;
        }
        if (defer && c.maxw * ((long long)rlen - 1) - 2ll * c.go >= S_) {  // (k = 1 is not ruled out by the potential: sweeps needed)
            r.verdict = CERT_DEFERRED;
            r.deferred = true;
            return r;
        }
        const long long n_ = (long long)rlen;
        uint32_t k = 1;
        for (; k < rlen; ++k) {
            if (c.maxw * (n_ - k) - 2ll * c.go - 2ll * c.ge * ((long long)k - 1) < S_) break;
            for (int dir = 0; dir < 2; ++dir) {
                if (cert_gapless_two_runs(wt, rlen, k, dir, c)) {
                    r.verdict = CERT_TWO_RUNS;
                    r.param = dir == 0 ? (int32_t)k : -(int32_t)k;
                    return r;
                }
            }
        }
        r.verdict = CERT_GAPLESS;
        r.param = (int32_t)(k - 1);
        return r;
    }
    const bool del = rlen > qlen;  // the run consumes reference rows
    const uint32_t g = del ? rlen - qlen : qlen - rlen, m = del ? qlen : rlen;
    const long long three_runs = c.maxw * m - 3ll * c.go - (long long)(g > 3 ? g - 3 : 0) * c.ge;
    if (!(m >= 2 && c.ge > 0 && S_ > three_runs)) {
        r.verdict = CERT_POTENTIAL;
        return r;
    }
    // second diagonal: the pairs behind the run
    const uint32_t dr = del ? g : 0, dq = del ? 0 : g;
    int64_t t1 = 0;
    for (uint32_t k = 0; k < m; ++k) t1 += wt(k + dr, k + dq);
    const int64_t gap = (int64_t)c.go + (int64_t)(g - 1) * c.ge;
    int64_t p0 = 0, p1 = 0, best = INT64_MIN;
    uint32_t best_p = 0, first_p = 0, n_best = 0;
    for (uint32_t p = 1; p < m; ++p) {
        p0 += wt(p - 1, p - 1);
        p1 += wt(p - 1 + dr, p - 1 + dq);
        const int64_t sc = p0 + (t1 - p1) - gap;
        if (sc > best) {
            best = sc;
            best_p = first_p = p;
            n_best = 1;
        } else if (sc == best) {
            ++n_best;
            best_p = p;  // the walk from the end takes the last
        }
    }
    r.param = (int32_t)best_p;
    r.ties = (int32_t)n_best;
    // one placement, or adjacent ones (a gap inside a homopolymer run)
    if (!(best_p - first_p == n_best - 1 && best == S_)) {
        r.verdict = CERT_PLACEMENT;
        return r;
    }
    // |ra| + |rb| <= X or the potential rules the pair out; |ra| + |gs - ra| >= 2 |ra| - g
    const long long gs = (long long)rlen - (long long)qlen;
    const long long X = (c.maxw * m - 2ll * c.go - S_) / c.ge + 2;
    const long long amax = X >= 0 ? (X + g) / 2 + 1 : 0;
    for (long long ra = -amax; ra <= amax; ++ra) {
        const long long rb = gs - ra;
        if (ra == 0 || rb == 0) continue;
        const long long ap = ra > 0 ? ra : 0, an = ra < 0 ? -ra : 0, bp = rb > 0 ? rb : 0, bn = rb < 0 ? -rb : 0;
        const long long M = (long long)rlen - ap - bp;
        if (M < 2) continue;
        const long long cost = 2ll * c.go + c.ge * (ap + an + bp + bn - 2);
        if (c.maxw * M - cost < S_) continue;
        if (defer) {
            r.verdict = CERT_DEFERRED;
            r.deferred = true;
            return r;
        }
        if (cert_one_gap_two_runs(wt, ap, an, bp, bn, M, cost, S_)) {
            r.verdict = CERT_TWO_RUNS;
            r.param = (int32_t)ra;
            return r;
        }
    }
    r.verdict = CERT_ONE_GAP;
    return r;
}

}  // namespace zsw
