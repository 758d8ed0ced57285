"""The texts the gzip kernels (reseq_amd/csrc/rsq_deflate.h) are tried on: named, seeded, at most about 550 KB each.  Every text is here for a path of the kernels:
a route (FASTQ by its lines / dense), a stored piece and why it is stored, a length at which a loop of the kernels begins or ends, a piece's end that the walk reads
across.  tests/test_device_gzip.py runs them through the host emulation (and asserts that they reach those paths) and through the kernels."""
import numpy as np

PIECE = 65280                  # gz::kPiece
ROUND = 8192                   # gz::kRound
RING = 16384                   # gz::kRing


def fastq_text(n_records, seed=1, read_len=150, quality_values=40):
    rng = np.random.default_rng(seed)
    recs = []
    pos = 1000
    for i in range(n_records):
        pos += int(rng.integers(0, 5))
        seq = bytes(b"ACGT"[c] for c in rng.integers(0, 4, read_len))
        q = rng.integers(0, quality_values, read_len)
        q[rng.random(read_len) < 0.6] = quality_values - 1                     # long runs of the best quality, as real reads have
        qual = bytes(int(x) + 35 for x in q)
        recs.append(b"@ReseqRead%d_%d:%d:synthEcoli0:%d:0:1337:1337 %dM E%d\n%s\n+\n%s\n" % (1 + i // 1000, i % 1000, pos, pos + 350 + int(rng.integers(0, 40)), read_len, int(rng.integers(0, 3)), seq, qual))
    return b"".join(recs)


def tiny_fastq_text(n_records, seed=2, line_end=b"\n"):
    """text like the test profile TINY's: reads of 30 bases that overlap their neighbours, five quality values"""
    rng = np.random.default_rng(seed)
    genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, 3000))
    recs = []
    pos = 0
    for i in range(n_records):
        pos = (pos + int(rng.integers(0, 3))) % (len(genome) - 30)
        qual = bytes(b"#,5:F"[c] for c in rng.integers(0, 5, 30))
        recs.append(b"@ReseqRead1_%d:%d:synthTiny0:%d:0:1337:1337 30M E0" % (i, pos, pos + 80) + line_end + genome[pos:pos + 30] + line_end + b"+" + line_end + qual + line_end)
    return b"".join(recs)


def quality_lines_that_begin_with_at(n_records, seed=4):
    """FASTQ whose quality lines begin with '@' (a legal quality character): by the rule for lines they are searched like id lines, and so is the id line behind them"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_records):
        seq = bytes(b"ACGT"[c] for c in rng.integers(0, 4, 100))
        qual = b"@" + bytes(int(x) + 64 for x in rng.integers(0, 6, 99))
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, seq, qual))
    return b"".join(recs)


def binary_records(n_records, seed=6):
    """40 random nibbles, four zero bytes, a counter: no line ends at all, bytes below 16 and runs of zeros"""
    rng = np.random.default_rng(seed)
    return b"".join(rng.integers(0, 16, 40, dtype=np.uint8).tobytes() + bytes(4) + i.to_bytes(4, "little") for i in range(n_records))


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def overflow_in_a_late_round():
    """four pieces of FASTQ; piece 1 is FASTQ for four rounds and random bytes from there on: the rounds of text are flushed into the member's slot before a round of
    random bytes needs more bits than the round's buffer holds, and the piece is stored over them"""
    fastq = fastq_text(800, seed=11)
    return fastq[:PIECE] + fastq[PIECE:PIECE + 4 * ROUND] + random_bytes(PIECE - 4 * ROUND, 12) + fastq[2 * PIECE:4 * PIECE]


def tail_text_t1(later=0):
    """A piece's end inside a searched line.  One line of 64 bytes, 1020 times, is exactly a piece; a '#' five bytes in front of the piece's end breaks the match that
    runs through the lines, so the position four bytes in front of the end is probed anew.  Its six-byte key takes its last two bytes from BEHIND the piece's end: in
    the kernel's ring that is the text 16384 bytes (256 lines) back, unless the ring is made a function of the piece.  `later`: bytes in front of the whole text, so
    that the '#' and the end of the line fall that much later against the piece's end."""
    rng = np.random.default_rng(21)
    line = b"@" + bytes(b"ACGTNacgtnRYKMSWBDHV"[c] for c in rng.integers(0, 20, 62)) + b"\n"
    piece = bytearray(line * (PIECE // 64))
    assert len(piece) == PIECE
    piece[PIECE - 5] = ord("#")
    return b"N" * later + bytes(piece) + line * 40


def tail_text_t2(later=0):
    """A short last piece that is no multiple of a segment and ends in a line that is not searched: "xIIII" is a byte, an 'I' and a run of three more.  The thread's
    segment is read whole, 32 bytes; an 'I' behind the end -- left in LDS by whatever workgroup ran before -- would make the run four bytes, long enough to be taken
    as a match (cut back to three), where the text alone gives three literals.  `later`: the tail begins that many bytes later."""
    lines = (b"ABCDEFGH" * 16)[:127] + b"\n"
    text = lines * 20
    return text[:len(text) - 64 + later] + b"xIIII"


def corpus():
    """[(name, text)]"""
    fastq = fastq_text(1500)
    texts = [
        ("fastq", fastq),
        ("tiny fastq", tiny_fastq_text(4000)),
        ("tiny fastq with CR LF", tiny_fastq_text(4000, line_end=b"\r\n")),
        ("quality lines that begin with @", quality_lines_that_begin_with_at(800)),
        ("one line of random bases", bytes(b"ACGT"[c] for c in np.random.default_rng(8).integers(0, 4, 200000))),
        ("lines of runs without @", (b"IIIIIIIIFFFFFFFF,,,,::::" * 8 + b"\n") * 1500),
        ("newlines only", b"\n" * 70000),
        ("lines of one @", b"@\n" * 40000),
        ("zero bytes", bytes(150000)),
        ("bytes 0xFF", b"\xff" * 150000),
        ("binary records", binary_records(5000)),
        ("overflow in a late round", overflow_in_a_late_round()),
        # the texts of test_edge_cases
        ("empty", b""),
        ("one byte", b"A"),
        ("three bytes", b"AAA"),
        ("a run longer than a match", b"G" * 5000),
        ("exactly a piece", bytes(range(256)) * 255),
        ("a piece and a byte", b"ACGT" * (PIECE // 4) + b"N"),
        ("a period longer than a group of positions", (b"0123456789abcdefghijklmnopqrstuvwxyz" * 10)[:300] * 400),
        ("text shorter than a hash window at a piece's end", b"x" * (PIECE - 2) + b"yz" + b"END"),
    ]
    # lengths at which a loop of the kernels begins or ends: a member no smaller than stored (10, 60), the CRC's slice per thread 0 or 1 bytes (255 .. 257), a round and
    # a byte more or less, a ring and a segment and a byte, a byte short of a piece
    for n in (10, 60, 255, 256, 257, ROUND - 1, ROUND + 1, RING + 33, PIECE - 1):
        texts.append((f"fastq cut to {n} bytes", fastq[:n]))
    for later in range(4):
        texts.append((f"T1 tail {later} later", tail_text_t1(later)))
        texts.append((f"T2 tail {later} later", tail_text_t2(later)))
    assert all(len(t) <= 550 << 10 for _, t in texts) and len({name for name, _ in texts}) == len(texts)
    return texts
