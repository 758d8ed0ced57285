"""NM:i and MD:Z of the truth alignments (rsq_sim_truth_md; reseq_amd/csrc/rsq_md.h): `md_nm`, the rule as include/reseq_amd.h states it, and what the tests of
the tags share -- the tags read from and taken off SAM lines and BAM records, so that what is left can be compared byte for byte with the records written with
the switch off, and `check_sam` / `check_bam`, which do both for a whole text.  The statement works from the finished record (POS, CIGAR, SEQ) and the
reference's bases alone."""
import re
import struct

_ELEMENT = re.compile(rb"(\d+)([MIDS])")
_TAGS = re.compile(rb"\tNM:i:(\d+)\tMD:Z:([0-9A-Z^]+)$")
_BAM_OPS = b"MIDNS"
_BAM_BASES = b"=ACMGRSVTWYHKDBN"


def md_nm(pos, cigar, seq, ref):
    """(NM, MD) of a mapped record: pos 1-based, cigar [(n, op)] with op in b"MIDS", seq and ref bytes"""
    r, q, run, nm, md = pos - 1, 0, 0, 0, b""
    for n, op in cigar:
        if op == b"M":
            for _ in range(n):
                if seq[q] == ref[r]:
                    run += 1
                else:
                    md += b"%d" % run + ref[r:r + 1]
                    run = 0
                    nm += 1
                q += 1
                r += 1
        elif op == b"I":
            q += n
            nm += n
        elif op == b"S":
            q += n
        elif op == b"D":
            md += b"%d" % run + b"^" + ref[r:r + n]
            run = 0
            r += n
            nm += n
        else:
            raise AssertionError(op)
    assert q == len(seq) and r <= len(ref)
    return nm, md + b"%d" % run


def parse_cigar(text):
    if text == b"*":
        return []
    elements = [(int(n), op) for n, op in _ELEMENT.findall(text)]
    assert b"".join(b"%d%s" % e for e in elements) == text, text
    return elements


def classes_of(nm, md, cigar, flag):
    """the classes of records a test wants to have met"""
    out = {"reverse" if flag & 0x10 else "forward"}
    if re.search(rb"[0-9][ACGT]", md):
        out.add("mismatch")
    if b"^" in md:
        out.add("deletion")
    if any(op == b"I" for _, op in cigar):
        out.add("insertion")
    if re.fullmatch(rb"\d+", md):
        out.add("no mismatch")
    if re.search(rb"[ACGT]0[ACGT^]", md) or re.search(rb"\^[ACGT]+0[ACGT]", md):
        out.add("0 separator")
    return out


def check_sam(tagged, plain, refs):
    """every mapped line of `tagged` carries the two tags and they are md_nm's, every unmapped one carries neither, and without them the text is `plain`, byte
    for byte.  refs: {RNAME: the sequence's bases}.  Returns {class: records}."""
    lines = tagged.split(b"\n")
    assert lines[-1] == b""
    stripped, seen = [], {}
    for line in lines[:-1]:
        f = line.split(b"\t")
        flag = int(f[1])
        m = _TAGS.search(line)
        if flag & 0x4:
            assert m is None and b"NM:i:" not in line and b"MD:Z:" not in line, line
            stripped.append(line)
            continue
        assert m is not None, b"a mapped record without the tags: " + line
        assert f[-2].startswith(b"NM:i:") and f[-1].startswith(b"MD:Z:")
        cigar = parse_cigar(f[5])
        want = md_nm(int(f[3]), cigar, f[9], refs[f[2]])
        assert (int(m.group(1)), m.group(2)) == want, (line, want)
        stripped.append(line[:m.start()])
        for c in classes_of(want[0], want[1], cigar, flag):
            seen[c] = seen.get(c, 0) + 1
    assert b"".join(l + b"\n" for l in stripped) == plain
    return seen


def bam_records(data):
    """the records of a stream of BAM records, each with its block_size field"""
    out, at = [], 0
    while at < len(data):
        (block_size,) = struct.unpack_from("<i", data, at)
        assert block_size >= 32 and at + 4 + block_size <= len(data)
        out.append(data[at:at + 4 + block_size])
        at += 4 + block_size
    return out


def bam_fields(rec):
    """what md_nm needs of a BAM record, and its tags: (refID, POS, flag, cigar, SEQ, [(tag, type, value, first byte, byte behind)])"""
    ref_id, pos, l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    at = 36 + l_read_name
    cigar = []
    for (w,) in struct.iter_unpack("<I", rec[at:at + 4 * n_cigar]):
        cigar.append((w >> 4, _BAM_OPS[w & 15:(w & 15) + 1]))
    at += 4 * n_cigar
    packed = rec[at:at + (l_seq + 1) // 2]
    seq = bytes(_BAM_BASES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    at += (l_seq + 1) // 2 + l_seq
    tags = []
    while at < len(rec):
        tag, kind, first = rec[at:at + 2], rec[at + 2:at + 3], at
        at += 3
        if kind == b"Z":
            end = rec.index(b"\0", at)
            value, at = rec[at:end], end + 1
        else:
            size = {b"S": 2, b"I": 4}[kind]
            value, at = int.from_bytes(rec[at:at + size], "little"), at + size
        tags.append((tag, kind, value, first, at))
    assert at == len(rec)
    return ref_id, pos + 1, flag, cigar, seq, tags


def check_bam(tagged, plain, refs):
    """check_sam for a stream of BAM records; refs: [the sequence's bases] by refID"""
    stripped, seen = [], {}
    for rec in bam_records(tagged):
        ref_id, pos, flag, cigar, seq, tags = bam_fields(rec)
        names = [t[0] for t in tags]
        if flag & 0x4:
            assert b"NM" not in names and b"MD" not in names
            stripped.append(rec)
            continue
        assert names[-2:] == [b"NM", b"MD"] and tags[-2][1] == b"I" and tags[-1][1] == b"Z", (names, b"a mapped record without the tags")
        want = md_nm(pos, cigar, seq, refs[ref_id])
        assert (tags[-2][2], tags[-1][2]) == want, (rec, want)
        cut = rec[4:tags[-2][3]]
        stripped.append(struct.pack("<i", len(cut)) + cut)
        for c in classes_of(want[0], want[1], cigar, flag):
            seen[c] = seen.get(c, 0) + 1
    assert b"".join(stripped) == plain
    return seen
