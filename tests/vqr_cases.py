"""Seeded rows and count vectors for the VQR tests (tests/test_vqr_cpu.py, tests/test_vqr_gpu.py), as the statement's dicts (tests/vqr_ref.py).
Everything the edge predicate and the categories can trip over is drawn often: runs of equal positions, gaps, coverage exactly at and one
below half a neighbour's, coverage 0, ForcedReport rows, N alleles, MNV / insertion / deletion rows."""
import numpy as np

from tests import vqr_ref as R

BASES = "ACGT"


def make_row(rng, position, coverage, snv_share=0.6, qscores=None):
    u = rng.random()
    ref = BASES[int(rng.integers(4))]
    if u < snv_share:
        alt = BASES[int(rng.integers(4))] if rng.random() > 0.05 else "N"   # alt == ref happens: a Reference by its strings
        if rng.random() < 0.03:
            ref = "N"
        t = "Snv"
    elif u < snv_share + 0.2:
        t, alt = "Reference", "."
    elif u < snv_share + 0.27:
        t, alt = "Insertion", ref + "GT"
    elif u < snv_share + 0.34:
        t, ref, alt = "Deletion", ref + "CA", ref
    else:
        t, ref, alt = "Mnv", "AC", "GT"
    bits = 0
    if rng.random() < 0.08:
        bits |= 1 << R.FILTER_FORCED_REPORT
    if rng.random() < 0.15:
        bits |= 1 << R.FILTER_LOW_VARIANT_QSCORE
    if rng.random() < 0.1:
        bits |= 1 << 4   # LowDP: any other bit must survive
    support = int(rng.integers(0, 2001)) if rng.random() < 0.8 else 0
    vq = int(rng.choice(qscores)) if qscores is not None else int(rng.integers(0, 101))
    return {"position": int(position), "total_coverage": int(coverage), "allele_support": support, "variant_qscore": vq,
            "genotype_qscore": int(rng.integers(0, 101)), "noise_level": 20, "filter_bits": bits, "type": t, "ref": ref, "alt": alt}


def make_rows(rng, n, snv_share=0.6, qscores=None, depths=None):
    """n rows of one chromosome in row order: positions that stay, step by one, or jump; coverage that holds, halves exactly, halves and
    loses one, or is 0"""
    rows = []
    position = int(rng.integers(1, 1000))
    level = int(rng.choice([10, 100, 101, 400, 3700]))
    for _ in range(n):
        u = rng.random()
        if u < 0.25:
            pass                                   # a run of equal positions
        elif u < 0.85:
            position += 1
        elif u < 0.93:
            position += 2                          # a hole of one
        else:
            position += int(rng.integers(3, 5000))
        u = rng.random()
        if u < 0.08:
            level = int(rng.choice([10, 100, 101, 400, 3700]))
        u = rng.random()
        if depths is not None:
            coverage = int(rng.choice(depths)) if rng.random() < 0.5 else int(rng.integers(0, 5001))
        elif u < 0.7:
            coverage = level
        elif u < 0.8:
            coverage = level // 2                  # exactly at the 0.5 boundary for an even level: no drop
        elif u < 0.9:
            coverage = max(0, (level + 1) // 2 - 1)   # one below it: a drop
        elif u < 0.95:
            coverage = 0
        else:
            coverage = 2 * level
        rows.append(make_row(rng, position, coverage, snv_share, qscores))
    return rows


def count_vector(rng):
    """(basic, edge) CountData for the tables: small counts with ties, zeros, all-equal vectors, edge equal to basic (0 / 0), no loci"""
    kind = int(rng.integers(8))
    def one():
        c = R.new_counts()
        if kind == 0:
            v = int(rng.integers(0, 50))
            for k in R.SNV_CATEGORIES:
                c["by"][k] = float(v)                                   # all equal: count == threshold, strictly above decides
        elif kind == 1:
            pass                                                        # zeros
        else:
            hi = int(rng.choice([3, 10, 1000, 10 ** 6]))
            for k in R.SNV_CATEGORIES:
                c["by"][k] = float(rng.integers(0, hi)) if rng.random() > 0.2 else 0.0
        for k in ("Insertion", "Deletion", "Other"):
            c["by"][k] = float(rng.integers(0, 30))
        c["npv"] = float(sum(c["by"].values()) + rng.integers(0, 10 ** 6)) if kind != 2 else 0.0   # kind 2: num_possible 0
        return c
    basic = one()
    if kind == 3:
        edge = {"by": dict(basic["by"]), "npv": basic["npv"]}           # edge == basic: 0 / 0 in the edge-risk rate
    else:
        edge = one()
        if kind >= 5:                                                   # a plausible pair: the edge rows are some of the rows
            for k in edge["by"]:
                edge["by"][k] = float(min(edge["by"][k], basic["by"][k]))
            edge["npv"] = float(min(edge["npv"], basic["npv"]))
    return basic, edge
