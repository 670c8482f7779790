"""The SAM line of one read, by string operations: the reference for the host model (tests/models/sam_line.cpp) and for
zsw_sam_batch on the device. What SamData::from_alignment + Display print (zoe_amd/records.py mirrors them), with the rules the
C ABI adds for caller-built records: a malformed record is an unmapped line."""

SOME = 0
OPS = b"MIDNSHP=X"


def malformed(rec, inc, op) -> bool:
    """rec: ciglet_offset / n_ciglets into the call's ciglet arrays inc / op"""
    off, n = int(rec["ciglet_offset"]), int(rec["n_ciglets"])
    if off > len(inc) or n > len(inc) - off:
        return True
    return any(int(inc[off + k]) == 0 or int(op[off + k]) not in OPS for k in range(n))


def sam_line(qname, seq: bytes, qual, status: int, rec, inc, op, rname: bytes, mapq: int = 255, strand: int = 0, stats=None, omit_seq: bool = False):
    """qname / qual: bytes, or None when the call has no such array; stats: (mismatches, ins_bases, del_bases) or None.
    -> (the line with its newline, whether the record counts as malformed)"""
    bad = status == SOME and malformed(rec, inc, op)
    name = b"*" if qname is None else bytes(qname)
    seq_field = b"*" if omit_seq or not seq else bytes(seq)
    qual_field = b"*" if qual is None or not seq else (bytes(qual)[::-1] if strand else bytes(qual))
    if status == SOME and not bad:
        off, n = int(rec["ciglet_offset"]), int(rec["n_ciglets"])
        cigar = b"".join(b"%d%c" % (int(inc[off + k]), int(op[off + k])) for k in range(n)) or b"*"
        fields = [name, b"16" if strand else b"0", bytes(rname), b"%d" % (int(rec["ref_start"]) + 1), b"%d" % mapq, cigar, b"*", b"0", b"0", seq_field, qual_field,
                  b"AS:i:%d" % int(rec["score"])]
        if stats is not None:
            fields.append(b"NM:i:%d" % (int(stats[0]) + int(stats[1]) + int(stats[2])))
    else:
        fields = [name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", seq_field, qual_field]
    return b"\t".join(fields) + b"\n", bad
