#!/usr/bin/env python3
"""Makes tests/golden/bam_scylla_chr21.npz from the reference's Scylla test data (src/test/Scylla.Tests/TestData), as data:
    bam           the bytes of chr21_11085587_S1.bam (what pisces_hip_bam_decode takes)
    ref_id        the index of chr21 in its header
    position ... quals   its chr21 records that are mapped, primary and carry a CIGAR, in file order, as PiscesReadBatch arrays
    mapq, flag    per such record
    vcf_position, vcf_ref, vcf_alt   the variant rows (ALT != .) of chr21_11085587_S1.genome.vcf, in file order
    python tests/golden/extract_scylla_fixture.py <reference root>      (or PISCES_REFERENCE=<reference root>)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extract_bam_fixture import read_bam  # noqa: E402

BAM = "src/test/Scylla.Tests/TestData/chr21_11085587_S1.bam"
VCF = "src/test/Scylla.Tests/TestData/chr21_11085587_S1.genome.vcf"
CHROM = "chr21"


def main(root):
    path = os.path.join(root, BAM)
    refs, reads = read_bam(path)
    keep = [r for r in reads if r["ref"] == CHROM and not (r["flag"] & 0x4) and not (r["flag"] & 0x100) and r["cigar"]]
    cigar_offset, seq_offset, ops, lens, bases, quals = [0], [0], [], [], [], []
    for r in keep:
        ops += [ord(o) for o, _ in r["cigar"]]
        lens += [n for _, n in r["cigar"]]
        bases.append(np.frombuffer(r["seq"].encode(), dtype=np.uint8))
        quals.append(r["qual"])
        cigar_offset.append(len(ops))
        seq_offset.append(seq_offset[-1] + len(r["seq"]))
    rows = []
    for line in open(os.path.join(root, VCF)):
        if line.startswith("#"):
            continue
        c = line.rstrip("\n").split("\t")
        if c[0] == CHROM and c[4] != ".":
            rows.append((int(c[1]), c[3], c[4]))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bam_scylla_chr21.npz")
    np.savez_compressed(
        dst, bam=np.frombuffer(open(path, "rb").read(), dtype=np.uint8), ref_id=np.int32(refs.index(CHROM)),
        position=np.array([r["pos"] for r in keep], dtype=np.int32), flags=np.array([(r["flag"] >> 4) & 1 for r in keep], dtype=np.uint8),
        cigar_offset=np.array(cigar_offset, dtype=np.int32), cigar_op=np.array(ops, dtype=np.uint8), cigar_len=np.array(lens, dtype=np.uint32),
        seq_offset=np.array(seq_offset, dtype=np.int32), bases=np.concatenate(bases), quals=np.concatenate(quals),
        mapq=np.array([r["mapq"] for r in keep], dtype=np.uint8), flag=np.array([r["flag"] for r in keep], dtype=np.uint16),
        vcf_position=np.array([p for p, _, _ in rows], dtype=np.int32), vcf_ref=np.array([r for _, r, _ in rows]), vcf_alt=np.array([a for _, _, a in rows]))
    clipped = sum(1 for r in keep if r["cigar"][0][0] == "S" or r["cigar"][-1][0] == "S")
    indel = sum(1 for r in keep if any(o in "ID" for o, _ in r["cigar"]))
    print(f"{len(keep)} of {len(reads)} records at {keep[0]['pos']}-{keep[-1]['pos']}, {clipped} soft-clipped, {indel} with an insertion or deletion; "
          f"{len(rows)} variant rows; {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["PISCES_REFERENCE"])
