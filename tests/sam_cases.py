"""The shape list of zsw_sam_batch's tests: hand-built reads and records at the edges of the formatter (decimal widths, sweeps of
64 ciglets, name lengths that move a line's start over every residue mod 16, read lengths around a sweep of lanes and around the
LDS cap of a line, every status, both strands, malformed records), shared by tests/test_sam_model.py (one case at a time through
the host model) and tests/test_gpu_sam.py (the list as one batch through the device). The expected text is tests/sam_ref.py."""
import numpy as np

import sam_ref

U32 = 2 ** 32 - 1
DIGIT_EDGES = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999,
               1000000000, U32]
DEC_VALUES = [0] + DIGIT_EDGES + [2 ** 32, 3 * U32, 10 ** 19 - 1, 10 ** 19, 2 ** 64 - 1]
RNAME = b"chrTest.1"

# what a call can leave out: (names, quals, strand, stats, omit_seq)
CONFIGS = [(True, True, True, True, False), (False, True, True, True, False), (True, False, True, True, False), (True, True, False, True, False),
           (True, True, True, False, False), (True, True, True, True, True), (True, False, False, False, True)]


def _bases(n, salt=0):
    return bytes(b"ACGTN"[(7 * k + salt + k // 5) % 5] for k in range(n))


def _quals(n, salt=0):
    return bytes(33 + (11 * k + salt) % 94 for k in range(n))


def _cig(n, salt=0):
    return [(DIGIT_EDGES[(k + salt) % len(DIGIT_EDGES)], sam_ref.OPS[(k + 2 * salt) % len(sam_ref.OPS)]) for k in range(n)]


def case(name=b"r", read=None, status=0, cig=None, strand=0, stats=(1, 2, 3), score=77, ref_start=11, offset=None, n_ciglets=None, salt=0):
    """cig: the record's own ciglets; offset / n_ciglets: a function of the call's ciglet total that replaces the record's real
    offset / count (malformed records)"""
    read = _bases(37, salt) if read is None else read
    return {"name": bytes(name), "read": bytes(read), "qual": _quals(len(read), salt), "status": status, "cig": _cig(2, salt) if cig is None else list(cig),
            "strand": strand, "stats": tuple(stats), "score": score, "ref_start": ref_start, "offset": offset, "n_ciglets": n_ciglets}


def line_of(c, rec, inc, op, cfg, rname=RNAME, mapq=255):
    names, quals, strand, stats, omit = cfg
    return sam_ref.sam_line(c["name"] if names else None, c["read"], c["qual"] if quals else None, c["status"], rec, inc, op, rname, mapq,
                            c["strand"] if strand else 0, c["stats"] if stats else None, omit)


def assemble(cases):
    """-> (records as a list of dicts, inc, op): the ciglets of all cases back to back, behind two ciglets that belong to nobody"""
    inc, op, recs = [5, 6], [ord("M"), ord("I")], []
    for c in cases:
        recs.append({"score": c["score"], "ref_start": c["ref_start"], "n_ciglets": len(c["cig"]), "ciglet_offset": len(inc)})
        inc += [i for i, _ in c["cig"]]
        op += [o for _, o in c["cig"]]
    for c, r in zip(cases, recs):
        if c["offset"] is not None:
            r["ciglet_offset"] = c["offset"](len(inc))
        if c["n_ciglets"] is not None:
            r["n_ciglets"] = c["n_ciglets"](len(inc))
    return recs, np.array(inc, dtype=np.uint32), np.array(op, dtype=np.uint8)


def malformed_cases():
    return [
        case(b"bad_beyond", offset=lambda t: t + 5, salt=1),                      # starts beyond the arrays
        case(b"bad_tail", offset=lambda t: t - 1, salt=2),                        # two ciglets, one of them inside
        case(b"bad_count", n_ciglets=lambda t: t + 1, offset=lambda t: 0, salt=3),
        case(b"bad_wrap", offset=lambda t: 2 ** 64 - 1, salt=4),                  # offset + n wraps 64 bits
        case(b"bad_wrap32", offset=lambda t: 2 ** 32, n_ciglets=lambda t: U32, salt=5),
        case(b"bad_inc0", cig=[(4, ord("M")), (0, ord("I")), (4, ord("M"))], salt=6),
        case(b"bad_op", cig=[(4, ord("M")), (3, ord("Z"))], salt=7),
        case(b"bad_op0", cig=[(4, 0)], salt=8),
        case(b"bad_op_late", cig=_cig(70) + [(1, ord("m"))], salt=9),             # found by the second sweep
        case(b"fine_unmapped_beyond", status=2, offset=lambda t: t + 5, salt=10),  # not SOME: the record is not looked at, not counted
    ]


def shape_cases(lds_cap, cfg=CONFIGS[0]):
    cs = []
    for k in range(32):  # names of 0..31 bytes in a row, the lines alike otherwise: each one byte longer, starts on every residue mod 16
        cs.append(case(bytes(65 + (k + j) % 26 for j in range(k))))
    for n in (0, 1, 63, 64, 65, 3000):
        cs.append(case(b"cig%d" % n, cig=_cig(n, n), salt=n))
    for n in (0, 1, 63, 64, 65):
        for s in (0, 1):
            cs.append(case(b"len%d_%d" % (n, s), read=_bases(n, n), strand=s, salt=n + s))
            cs.append(case(b"ulen%d_%d" % (n, s), read=_bases(n, n + 1), strand=s, status=2, salt=n + s))
    for st in (0, 1, 2, 3, 4, 255):
        cs.append(case(b"status%d" % st, status=st, salt=st))
    cs.append(case(b"wide", score=U32, ref_start=U32, stats=(U32, U32, U32), strand=1))
    cs.append(case(b"zero", score=0, ref_start=0, stats=(0, 0, 0)))
    cs.append(case(b"nine", score=9, ref_start=8, stats=(3, 3, 3)))
    cs.append(case(b"ten", score=10, ref_start=9, stats=(10, 0, 0)))
    for target in (lds_cap - 1, lds_cap, lds_cap + 1, 2 * lds_cap + 3):  # lines one byte each side of the LDS cap (under cfg)
        for s in (0, 1):
            probe = case(b"cap", read=_bases(1), strand=s)
            recs, inc, op = assemble([probe])
            base = len(line_of(probe, recs[0], inc, op, cfg)[0])
            per_base = len(line_of(case(b"cap", read=_bases(2), strand=s), recs[0], inc, op, cfg)[0]) - base
            if per_base == 0:
                continue
            extra = (target - base) % per_base
            c = case(b"cap" + b"x" * extra, read=_bases(1 + (target - base - extra) // per_base, target), strand=s)  # the probes' salt: the same ciglets
            cs.append(c)
    return cs + malformed_cases()
