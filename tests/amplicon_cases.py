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


def names_of(ids):
    return [None if i < 0 else i for i in ids]
