"""The read scenarios of tests/test_amplicon_gpu.py as data (no device, no library): tests/test_amplicon_cpu.py reads them too, to assert
from the Python statement alone that no decision they lead to sits on its threshold."""
import numpy as np

THRESHOLD = 0.01
AMP_A, AMP_B = 3, 8            # ids are the host's choice: not 0 / 1, not adjacent
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def reference(length=1400, seed=11):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(list(b"ACGT"), length).astype(np.uint8))


def _read(ref, pos, cigar, reverse=False, edits=(), low=(), qual=35):
    """A read that matches the reference except at `edits` {position: base}; `low`: positions whose base gets quality 5"""
    seq, quals, p = [], [], pos
    for op, n in cigar:
        if op in "M":
            for k in range(n):
                seq.append(edits.get(p + k, chr(ref[p + k - 1])) if edits else chr(ref[p + k - 1]))
                quals.append(5 if (p + k) in low else qual)
            p += n
        elif op in "IS":
            seq += ["G"] * n
            quals += [qual] * n
        elif op in "DN":
            p += n
    return dict(pos=pos, cigar=list(cigar), seq="".join(seq), quals=bytes(quals), reverse=reverse)


def counts_scenario():
    """Three overlapping amplicons of 150 reads each over 940..1090 (a 64-locus tile edge at 960 / 1024 and the block edge at 1000 inside):
    reads without a tag, low-quality and N bases, soft clips, insertions, deletions, one reverse-strand group; and fourteen reads with two
    gaps and no aligned base between them (40M3D2I2D53M), which the store keeps without fragments and walks base by base.
    -> (ref, reads, ids), in position order."""
    ref = reference()
    rng = np.random.default_rng(5)
    reads, ids = [], []
    for amp, start in ((21, 940), (4, 965), (13, 991)):
        for i in range(150):
            kind = i % 6
            cigar = {0: [("M", 100)], 1: [("S", 5), ("M", 95)], 2: [("M", 40), ("I", 2), ("M", 58)], 3: [("M", 50), ("D", 3), ("M", 47)],
                     4: [("M", 97), ("S", 3)], 5: [("M", 100)]}[kind]
            span = sum(n for op, n in cigar if op in "MD")
            edits = {int(p): str(rng.choice(list("ACGTN"))) for p in rng.integers(start, start + span, 3)}
            low = set(int(p) for p in rng.integers(start, start + span, 4))
            reads.append(_read(ref, start, cigar, reverse=(amp == 4), edits=edits, low=low))
            ids.append(-1 if i % 7 == 0 else amp)
    rng = np.random.default_rng(6)
    for i in range(14):
        amp, start = ((21, 945), (13, 998))[i & 1]
        edits = {int(p): str(rng.choice(list("ACGTN"))) for p in rng.integers(start, start + 98, 3)}
        low = set(int(p) for p in rng.integers(start, start + 98, 4))
        reads.append(_read(ref, start, GAP_CHAIN, reverse=bool(i & 2), edits=edits, low=low))
        ids.append(-1 if i % 7 == 0 else amp)
    order = sorted(range(len(reads)), key=lambda k: reads[k]["pos"])
    return ref, [reads[k] for k in order], [ids[k] for k in order]


GAP_CHAIN = [("M", 40), ("D", 3), ("I", 2), ("D", 2), ("M", 53)]


def high_threshold_scenario():
    """min_base_call_quality = 130, above what a row code's low-quality bit can hold (the store encodes it against 127): two amplicons of
    twelve reads over 950..1049 whose qualities are 140 (counted), 128 (above 127, below the threshold: not counted) and 5, one read in four
    with the two-gap CIGAR.  -> (ref, reads, ids, min_base_call_quality)"""
    ref = reference()
    rng = np.random.default_rng(7)
    reads, ids = [], []
    for i in range(24):
        r = _read(ref, 950, GAP_CHAIN if i % 4 == 3 else [("M", 100)], reverse=bool(i & 2))
        r["quals"] = bytes(rng.choice([140, 128, 5], len(r["seq"]), p=[0.6, 0.3, 0.1]).astype(np.uint8))
        reads.append(r)
        ids.append((2, 9)[i & 1])
    return ref, reads, ids, 130


# what the filter scenario plants: position -> (what, expected decision of the Python statement for the SNV row there)
PLANTED = {120: ("10 % in A, 0 % in B", True), 125: ("50 % in A, 0 % in B: a het call of the diploid genotyper too", True), 140: ("10 % in A, 9 % in B", False), 160: ("carriers untagged", None), 180: ("deletion in A only", "no SNV row"),
           230: ("one amplicon covers the locus", None)}


def filter_scenario():
    """Two amplicons (ids AMP_A, AMP_B) at 200x each over 100..199, amplicon A alone at 200x over 200..259, 20 untagged reads over 100..199.
    -> (ref, reads, ids), in position order."""
    ref = reference()
    alt = lambda p: OTHER[chr(ref[p - 1])]
    reads, ids = [], []
    for i in range(200):
        edits = {}
        if i < 20:
            edits[120] = alt(120)
            edits[140] = alt(140)
        if 40 <= i < 140:
            edits[125] = alt(125)
        cigar = [("M", 80), ("D", 1), ("M", 19)] if 20 <= i < 40 else [("M", 100)]   # the deletion covers position 180
        reads.append(_read(ref, 100, cigar, reverse=bool(i & 1), edits=edits))
        ids.append(AMP_A)
    for i in range(200):
        edits = {140: alt(140)} if i < 18 else {}
        reads.append(_read(ref, 100, [("M", 100)], reverse=bool(i & 1), edits=edits))
        ids.append(AMP_B)
    for i in range(20):
        reads.append(_read(ref, 100, [("M", 100)], reverse=bool(i & 1), edits={160: alt(160)}))
        ids.append(-1)
    for i in range(200):
        reads.append(_read(ref, 200, [("M", 60)], reverse=bool(i & 1), edits={230: alt(230)} if i < 20 else {}))
        ids.append(AMP_A)
    order = sorted(range(len(reads)), key=lambda k: reads[k]["pos"])
    return ref, [reads[k] for k in order], [ids[k] for k in order]


# the haploid genotyper reports a variant only as the locus' one allele (above 70 %, the reference below 20 %): position -> expected decision
HAPLOID_PLANTED = {120: True, 140: False, 160: False}


def haploid_scenario():
    """Amplicon A at 300x and amplicon B at 40x over 100..199: 120 every read of A and none of B, 140 every read of both,
    160 290 reads of A and 38 of B (both above the 10 % that pass freely).  -> (ref, reads, ids), in position order."""
    ref = reference()
    alt = lambda p: OTHER[chr(ref[p - 1])]
    reads, ids = [], []
    for amp, depth, carriers_160 in ((AMP_A, 300, 290), (AMP_B, 40, 38)):
        for i in range(depth):
            edits = {140: alt(140)}
            if amp == AMP_A:
                edits[120] = alt(120)
            if i < carriers_160:
                edits[160] = alt(160)
            reads.append(_read(ref, 100, [("M", 100)], reverse=bool(i & 1), edits=edits))
            ids.append(amp)
    return ref, reads, ids


def names_of(ids):
    return [None if i < 0 else i for i in ids]


# ---- seeded generators (the fuzz of tests/test_amplicon_gpu.py; their promises are asserted from the data in tests/test_amplicon_cpu.py) ----

TAGGED_SEEDS = [101, 202]
WINDOW = 200                       # above the longest reference span random_reads can make (189: six operations of 29, M5, two deletions of 5)
IDS_A_WINDOW = (3, 2, 1, 2, 1, 3)  # by window % 6: the windows 4..8 of 940..1639 hold 1, 3, 3, 2, 1 ids, so neighbours add up to 4, 6, 5, 3
ID_POOL = (0, 7, 12, 0x7FFFFFFF, 65535, 1 << 30, 65536, 0x7FFFFFFE, 1, 100003, 255, 31)   # twelve distinct: two neighbouring windows never share an id
FUZZ_LO, FUZZ_HI = 940, 1640
FUZZ_REF_LENGTH = 68000


def window_ids(position):
    """The ids a read that starts at `position` may carry: a position sees reads of its own window and of the one before, six ids at the most"""
    w = position // WINDOW
    return [ID_POOL[(3 * w + i) % len(ID_POOL)] for i in range(IDS_A_WINDOW[w % 6])]


def ref_span(read):
    return sum(n for op, n in read["cigar"] if op in "M=XDN")


def _random_bases(rng, cigar):
    n = sum(length for op, length in cigar if op in "MIS=X")
    return (bytes(rng.choice(list(b"ACGTN"), n, p=[.24, .24, .24, .24, .04]).astype(np.uint8)),
            rng.choice([10, 25, 37, 200], n, p=[.15, .2, .63, .02]).astype(np.uint8).tolist())


def _extra_read(rng, pos, cigar):
    seq, quals = _random_bases(rng, cigar)
    return {"pos": int(pos), "cigar": list(cigar), "seq": seq, "quals": quals, "reverse": bool(rng.integers(0, 2))}


def random_tagged_reads(seed, n=600, lo=FUZZ_LO, hi=FUZZ_HI, exotic=False, tag_all=False, ref_length=FUZZ_REF_LENGTH, extras=True):
    """tests.test_read_store.random_reads over [lo, hi) with an id per read: one read in seven without a tag (none with tag_all), the others
    one of window_ids(read position), so that no position ever sees a seventh id.  extras: six reads whose span exceeds 0xFFFF through one
    long N (one of them ends on the reference's last base), four reads that start at position 1, four that end on the last base.
    -> (reads, ids) in the order drawn (the callers sort or do not)."""
    from tests.test_read_store import random_reads
    rng = np.random.default_rng(seed)
    reads = random_reads(rng, n, lo, hi, exotic=exotic, sort=False)
    if extras:
        for i in range(6):
            pos = int(rng.integers(1010, 1190))          # one window: at most three ids travel to the far end
            a, b = int(rng.integers(5, 40)), int(rng.integers(5, 40))
            gap = 66000 + int(rng.integers(0, 300)) if i else ref_length - pos - a - b + 1
            reads.append(_extra_read(rng, pos, [("M", a), ("N", gap), ("M", b)] if i != 3 else [("S", 3), ("M", a), ("N", gap), ("M", b), ("I", 2), ("M", 4)]))
        for i in range(4):
            reads.append(_extra_read(rng, 1, [("M", int(rng.integers(20, 120)))] if i != 2 else [("S", 4), ("M", 30), ("D", 2), ("M", 30)]))
        for i in range(4):
            cigar = [("M", int(rng.integers(20, 120)))] if i != 2 else [("M", 30), ("I", 1), ("M", 30), ("S", 4)]
            reads.append(_extra_read(rng, ref_length - sum(n for op, n in cigar if op == "M") + 1, cigar))
    ids = []
    for i, r in enumerate(reads):
        pool = window_ids(r["pos"])
        ids.append(-1 if (i % 7 == 3 and not tag_all) else int(pool[int(rng.integers(0, len(pool)))]))
    return reads, ids


def further_tagged_reads(seed, lo, hi, n=60, shift=0):
    """A later batch over [lo, hi): ordinary reads, every one tagged; shift: the ids of the window `shift` windows further on (other ids over the
    same positions, for a store that holds nothing else there)"""
    from tests.test_read_store import random_reads
    rng = np.random.default_rng(seed)
    reads = random_reads(rng, n, lo, hi, sort=True)
    ids = []
    for r in reads:
        pool = window_ids(r["pos"] + shift * WINDOW)
        ids.append(int(pool[int(rng.integers(0, len(pool)))]))
    return reads, ids


PLANTED_THRESHOLDS = (0.01, 0.001, 0.05, 0.2, 0.5)
PLANTED_SEEDS = [(31, 0.01), (32, 0.001), (33, 0.05), (34, 0.2), (35, 0.5)]     # (seed, threshold)
MIN_FREQUENCY = 0.01               # the callers' default (MinimumFrequency)
VARIANT_FREQUENCIES = (0.005, 0.01, 0.02, 0.05, 0.08, 0.1, 0.12, 0.3)     # seeded_sets' (tests/test_amplicon_cpu.py)
DEPLETION = (0.0, 0.3, 0.6, 0.8, 1.0, 1.1)
DEPTHS, DEPTH_P = (30, 60, 120, 250, 500, 1000), (.22, .22, .22, .18, .10, .06)


def _poisson_tail(k, lam):
    """P(X >= k) for X ~ Poisson(lam)"""
    import math
    term, cdf = math.exp(-lam), 0.0
    for i in range(k):
        cdf += term
        term *= lam / (i + 1)
    return max(0.0, 1.0 - cdf)


def is_special(p):
    """The first, the last and the last-but-one position of a 64-locus tile, or the first position of a block.  Tiles start at a block's
    first position and blocks at 1 + a multiple of 1000: in the first block these are p % 64 in (1, 0, 63)."""
    offset = (p - 1) % 1000
    return offset % 64 in (0, 63, 62)


def planted_scenario(seed, threshold):
    """filter_scenario at large: eight regions of 100-base reads — one at position 1, six between 905 and 1780 (the block edge 1000 / 1001 inside
    the first) with 1..6 amplicons in a seeded order, one that ends on the reference's last base — every amplicon at its own depth (tens to
    about a thousand) and its own offset, untagged reads (20-40 and a twentieth of the region's depth), two low-quality bases a read.  Each region has about ten planted
    loci at least 7 apart, the tile edges and block starts of the region among them.  A locus draws one variant frequency and a depletion
    factor per amplicon (seeded_sets' distributions) and its carriers from them; one locus in six plants a second alternative base, one in
    eight has its carriers among the untagged reads; position 1, the last base and a block's first position always carry an allele of 2.5 %
    or more.  A draw whose allele would reach 1.5 % of the depth without the support a call
    needs (Poisson tail of the 1 % noise above 1e-3) is drawn again, so that every allele of 2 % and more has its row.
    -> dict(ref, reads, ids (position order), threshold, loci: {position: dict(k, alts: [base...], untagged: bool)})"""
    rng = np.random.default_rng(seed)
    ks = [int(k) for k in rng.permutation(6) + 1]
    starts = [1] + [905 + 150 * r + int(rng.integers(0, 16)) for r in range(6)] + [1850]
    ks = [int(rng.integers(2, 5))] + ks + [int(rng.integers(2, 5))]
    length = starts[-1] + 99
    ref = reference(length)
    all_ids = [0, 0x7FFFFFFF] + [int(x) + 1 for x in rng.choice(10 ** 6, 40, replace=False)]
    all_ids = [all_ids[i] for i in rng.permutation(len(all_ids))]
    reads, ids, loci = [], [], {}
    for region, (start, k) in enumerate(zip(starts, ks)):
        edge = region in (0, len(starts) - 1)
        offsets = [0] * k if edge else [int(o) for o in rng.integers(0, 9, k)]
        amps = [all_ids.pop() for _ in range(k)]
        depths = [max(20, int(rng.choice(DEPTHS, p=DEPTH_P) * rng.uniform(0.7, 1.3))) for _ in range(k)]
        n_untagged = int(rng.integers(20, 41)) + sum(depths) // 20
        # the region's reads as (start, id, edits); the untagged ones last
        members = [[(start + off, amp, {}) for _ in range(depth)] for off, amp, depth in zip(offsets, amps, depths)]
        members.append([(start + (0 if edge else 4), -1, {}) for _ in range(n_untagged)])
        core_lo, core_hi = (start, start + 99) if edge else (start + 8, start + 99)
        grid = [core_lo + 9 * i + (0 if edge else int(rng.integers(0, 3))) for i in range(12)]
        grid = [p for p in grid if p <= core_hi]
        chosen, group = [], []
        for p in range(core_lo, core_hi + 2):
            if p <= core_hi and is_special(p) and not edge:
                group.append(p)
            elif group:
                chosen.append(int(rng.choice(group)))
                group = []
        positions = sorted(set(chosen) | {p for p in grid if all(abs(p - q) >= 7 for q in chosen)})
        total_depth = sum(depths) + n_untagged
        for p in positions:
            n_alts = 2 if rng.integers(0, 6) == 0 else 1
            must = p in (1, length) or p % 1000 == 1      # position 1, the last base, a block's first position: always an allele with a row
            untagged = bool(rng.integers(0, 8) == 0) and not must
            alts = [b for b in "ACGT" if b != chr(ref[p - 1])]
            alts = [alts[i] for i in rng.permutation(3)[:n_alts]]
            free = [list(rng.permutation(len(m))) for m in members]     # reads of every group that carry no allele here yet
            for alt in alts:
                for _ in range(50):
                    if untagged:
                        carriers = [0] * k + [int(rng.integers(n_untagged // 4, n_untagged // 2))]
                    else:
                        vf = float(rng.choice(VARIANT_FREQUENCIES))
                        keep = rng.choice(DEPLETION, size=k)
                        carriers = [int(min(len(free[j]), rng.poisson(depths[j] * vf * keep[j]))) for j in range(k)] + [0]
                    s = sum(carriers)
                    if must and alt == alts[0] and s < 0.025 * total_depth:
                        continue
                    if s == 0 or s < 0.015 * total_depth or _poisson_tail(s, MIN_FREQUENCY * total_depth) <= 1e-3:
                        break
                else:
                    carriers = [0] * (k + 1)
                for j, c in enumerate(carriers):
                    for _ in range(c):
                        members[j][free[j].pop()][2][p] = alt
            loci[p] = dict(k=k, alts=alts, untagged=untagged)
        for m in members:
            for i, (pos, amp, edits) in enumerate(m):
                low = set(int(x) for x in rng.integers(pos, pos + 100, 2))
                reads.append(_read(ref, pos, [("M", 100)], reverse=bool(i & 1), edits=edits, low=low))
                ids.append(amp)
    order = sorted(range(len(reads)), key=lambda i: reads[i]["pos"])
    return dict(ref=ref, reads=[reads[i] for i in order], ids=[ids[i] for i in order], threshold=threshold, loci=loci)


def lifecycle_case(seed, exotic=False, tag_all=False):
    """What the counts fuzz adds over a store's life: the reads of random_tagged_reads; a position to call up to that is no block edge and
    the floor that call leaves (the first position of the block it lies in); a tagged batch that straddles the floor (its first reads start
    below it, in the block the call cleared); and, for after the final call, a batch with other ids over the same positions."""
    reads, ids = random_tagged_reads(seed, exotic=exotic, tag_all=tag_all)
    call_at = int(np.random.default_rng(seed + 1).integers(1100, 1600))
    floor = call_at // 1000 * 1000 + 1
    return dict(reads=reads, ids=ids, call_at=call_at, floor=floor, ahead=further_tagged_reads(seed + 2, floor - 40, floor + 400),
                fresh=further_tagged_reads(seed + 3, FUZZ_LO, FUZZ_HI, n=120, shift=1))
