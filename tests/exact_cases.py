"""Reads and spans for the device tests of CoverageMethod.Exact (tests/test_exact_gpu.py): seeded reads with arbitrary CIGARs and per-base
directions plus the hand-made reads of the named cases, and the spans that ask them.  Every base has quality 37, so every gap passes
CheckDeletionQuality and the statement's blocks (tests/exact_ref.py) are the library's."""
import random

from tests import exact_ref as R

BLOCK = 100
REF_LEN = 2000          # the last base of the reference the reads are laid on
FIRST_READ_LEN = 20     # the handle's first read: RegionStateManager._readLength, so the look-forward window is 40 positions


def _seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def make_read(rng, pos, cigar, dirs=None, reverse=False):
    cigar = R.parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    n = sum(k for op, k in cigar if op in R.READ_SPAN)
    rd = {"pos": int(pos), "cigar": cigar, "seq": _seq(rng, n), "quals": [37] * n, "reverse": bool(reverse)}
    if dirs is not None:
        assert len(dirs) == n
        rd["dirs"] = list(dirs)
    return rd


def directions_of(read):
    """SequencedBaseDirectionMap as the library takes it: the per-base directions, or the flag's for every base"""
    n = len(read["seq"])
    return read["dirs"] if read.get("dirs") is not None else [R.REVERSE if read["reverse"] else R.FORWARD] * n


def stitched(rng, n):
    """F.. S.. R.. (1-4 runs in general: some reads drop a part or repeat one)"""
    k = rng.choice((2, 3, 3, 3, 4))
    cuts = sorted(rng.sample(range(1, n), k - 1)) if n > k else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    order = {2: rng.choice(((0, 2), (2, 1), (0, 1))), 3: (0, 2, 1), 4: (0, 2, 1, 2)}[len(lens)] if len(lens) > 1 else (rng.randrange(3),)
    return [d for d, m in zip(order, lens) for _ in range(m)]


def random_cigar(rng):
    ops = []
    if rng.random() < 0.1:
        ops.append(("H", rng.randint(1, 4)))
    if rng.random() < 0.3:
        ops.append(("S", rng.randint(1, 12)))
    if rng.random() < 0.1:
        ops.append(("I", rng.randint(1, 4)))
    body = rng.randint(1, 4)
    for k in range(body):
        ops.append((rng.choice("MMM=X"), rng.randint(4, 45)))
        if k + 1 < body:
            r = rng.random()
            ops.append(("I", rng.randint(1, 6)) if r < 0.4 else ("D", rng.randint(1, 8)) if r < 0.8 else ("N", rng.randint(1, 30)) if r < 0.92 else ("P", 2))
    if rng.random() < 0.1:
        ops.append(("I", rng.randint(1, 4)))
    if rng.random() < 0.06:
        ops.append(("D", rng.randint(1, 4)))
    if rng.random() < 0.3:
        ops.append(("S", rng.randint(1, 12)))
    if rng.random() < 0.1:
        ops.append(("H", rng.randint(1, 4)))
    return ops


def named_reads(rng):
    """The reads the named cases need, whatever the seed gives: label -> read"""
    return {
        "ends at preceding in an insertion": make_read(rng, 300, "30M5I", stitched(rng, 35)),
        "ends at preceding, no insertion": make_read(rng, 300, "30M"),
        "ends at preceding, insertion then clip": make_read(rng, 300, "30M3I2S"),
        "starts at trailing in an insertion": make_read(rng, 400, "5I30M", reverse=True),
        "starts at trailing, no insertion": make_read(rng, 400, "30M"),
        "several directions behind a leading clip": make_read(rng, 500, "6S40M", [0] * 10 + [2] * 20 + [1] * 16),
        "trailing clip alone reaches the next block": make_read(rng, 590, "8M5S", [0] * 13),
        "reference span above 0xFFFF": make_read(rng, 700, "12M70000N12M", [0] * 8 + [2] * 8 + [1] * 8),
        "at position 1 behind a clip": make_read(rng, 1, "4S30M", [0] * 10 + [2] * 10 + [1] * 14),
        "ends at the reference's last base": make_read(rng, REF_LEN - 29, "30M4S", reverse=True),
    }


NAMED_SPANS = {
    "ends at preceding in an insertion": (329, 330),
    "starts at trailing in an insertion": (399, 400),
    "several directions behind a leading clip": (497, 501),       # through the shifted map: index of 497 is 9 -> ... ; from Position it would differ
    "trailing clip alone reaches the next block": (598, 599),
    "reference span above 0xFFFF": (40000, 40003),
    "at position 1 behind a clip": (1, 2),
    "ends at the reference's last base": (REF_LEN - 1, REF_LEN),
}


def counts_scenario(seed=7, n_random=330, n_pile=140):
    """(first read, reads sorted by position, named reads).  The pile: n_pile reads over 1000 .. 1045, so that more than 128 reads span one span."""
    rng = random.Random(seed)
    first = make_read(rng, 1, f"{FIRST_READ_LEN}M")
    reads = []
    for i in range(n_random):
        cigar = random_cigar(rng)
        ref_span = sum(k for op, k in cigar if op in R.REF_SPAN)
        n = sum(k for op, k in cigar if op in R.READ_SPAN)
        pos = rng.randint(1, max(1, min(1500, REF_LEN - ref_span)))
        reads.append(make_read(rng, pos, cigar, stitched(rng, n) if (i % 2 == 0 and n > 4) else None, reverse=bool(i % 3 == 0)))
    for i in range(n_pile):
        reads.append(make_read(rng, 1000 + i % 6, "40M", stitched(rng, 40) if i % 4 == 0 else None, reverse=bool(i & 1)))
    named = named_reads(rng)
    reads += list(named.values())
    reads.sort(key=lambda r: r["pos"])
    return first, reads, named


def indel_spans(read):
    """The spans the read's own insertions and deletions ask with, as candidates of a flush (ExactCoverageCalculator.Compute :18-42)"""
    out, ref = [], read["pos"]
    for op, length in read["cigar"]:
        if op == "D":
            out.append(R.span_of("deletion", ref - 1, length))
        elif op == "I":
            out.append(R.span_of("insertion", ref - 1, length))
        if op in R.REF_SPAN:
            ref += length
    return [sp for sp in out if sp[0] >= 1]


def spans_for(reads, seed=11, per_read=1):
    """Spans at every relation to reads' ends: around CS, CE, Position, EndPosition of a sample of reads, lengths 1 .. 30, and the named ones"""
    rng = random.Random(seed)
    spans = set(NAMED_SPANS.values()) | {(1008, 1009), (1010, 1014)}
    named_cigars = [rd["cigar"] for rd in named_reads(random.Random(0)).values()]
    for k, rd in enumerate(reads):
        if k % 3 and rd["cigar"] not in named_cigars:
            continue
        s = R.Summary.of_read(rd["pos"], rd["cigar"], directions_of(rd))
        ref_span = sum(k for op, k in rd["cigar"] if op in R.REF_SPAN)
        anchors = (s.cs, s.ce, rd["pos"], rd["pos"] + ref_span - 1, (s.cs + s.ce) // 2)
        for _ in range(per_read):
            a = max(rng.choice(anchors) + rng.randint(-2, 2), 1)
            spans.add((a, a + rng.choice((1, 1, 2, 3, 5, 9, 30))))
        spans.add((max(s.ce, 1), max(s.ce, 1) + 1))     # a read ending exactly at `preceding`
        spans.add((max(s.cs - 1, 1), max(s.cs, 2)))     # a read starting exactly at `trailing`
    return sorted(sp for sp in spans if sp[0] < 75000)
