"""Layouts for the RMxN filter tests (tests/test_rmxn_cpu.py, tests/test_rmxn_gpu.py) — TEST INFRASTRUCTURE, no tests in here.

A layout is one chromosome and the alleles laid out on it; what a run returns for it is {allele key: FILTER_RMXN bit}, and what it must
return is tests/rmxn_ref.py's answer for the row's own support and coverage.  Here: the reference's table (tests/golden/rmxn_cases.json),
the directed SNV grid (tile edges, the eight-neighbour shortcut, the LDS margin, chromosome ends, N, the frequency limit), the directed
spanning grid (unit lengths, bookends, the ratchet, chromosome ends), the seeded generator, and the oracle's side of all of them.
"""
import json
import os
from types import SimpleNamespace

import numpy as np

from pisces_amd import _abi
from tests import orc, rmxn_ref

G = os.path.join(os.path.dirname(__file__), "golden")
TILE, BLOCK = 64, 1000          # loci of a tile; positions of a block of the streaming surface (tiles start anew with every block)
COV = 20                        # flat coverage of every layout
OVERHANG = 16                   # loci with counts behind the last base where a table case is the whole chromosome
ANCHOR = _abi.ANCHOR_SIZE       # every observation is well anchored
CAT = {"Snv": _abi.CAT_SNV, "Mnv": _abi.CAT_MNV, "Insertion": _abi.CAT_INSERTION, "Deletion": _abi.CAT_DELETION}
CAT_NAME = {v: k for k, v in CAT.items()}
LIMIT = 0.35                    # the default RMxNFilterFrequencyLimit
F32 = np.float32


def config(max_unit, min_rep, limit=LIMIT, **kw):
    """Every candidate comes back as a row and no other filter is on: MNV calling on, the collapser off."""
    base = dict(min_coverage=0, min_variant_qscore=0, min_frequency=0.0, variant_qscore_filter=-1, low_depth_filter=-1, variant_freq_filter=-1.0,
                no_call_filter_threshold=-1.0, low_gq_filter=-1, include_reference_calls=0, collapse=0, call_mnvs=1, max_mnv_length=8,
                rmxn_max_repeat_length=max_unit, rmxn_min_repetitions=min_rep, rmxn_frequency_limit=float(limit))
    base.update(kw)
    return _abi.default_config(**base)


def allele(category, position, ref, alt, support=4, name=None, from_counts=None, no_row=False):
    """from_counts: the allele's support stands in the allele counts (SNVs, by default) and not in a candidate.  no_row: observations
    that must not become a row at all (an alternate base over a reference N: no candidate is made there, so nothing is there to filter)."""
    return SimpleNamespace(category=category, position=position, ref=ref, alt=alt, support=support, name=name, no_row=no_row,
                           from_counts=(category == "Snv") if from_counts is None else from_counts)


def key_of(a):
    return (a.category, a.position, a.ref, a.alt)


def expected_bits(chrom, alleles, max_unit, min_rep, limit, counts_of):
    """The statement's answer for every allele; counts_of: {key: (support, coverage)} as the rows report them."""
    out = {}
    for a in alleles:
        if a.no_row:
            continue
        s, c = counts_of[key_of(a)]
        out[key_of(a)] = int(rmxn_ref.should_filter(a.category, a.position, a.ref, a.alt, chrom, max_unit, min_rep, F32(limit), s, c))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# counts, observations, tiles, reads of a layout
# ------------------------------------------------------------------------------------------------------------------------------------
def folded_counts(chrom, alleles, overhang=0):
    """int32[len + overhang][6][3]: COV forward observations of the reference base at every position (of A where it is N: an allele
    anchored there has its coverage too; and on `overhang` loci behind the last base, for the deletions of the reference's table that
    reach past their sequence), the support of the alleles that come from counts moved to their alternate base."""
    n = len(chrom) + overhang
    counts = np.zeros((n, 6, 3), np.int32)
    codes = np.array([_abi.ALLELE_OF_BASE[b] for b in chrom.replace("N", "A") + "A" * overhang])
    counts[np.arange(n), codes, 0] = COV
    for a in alleles:
        if a.from_counts:
            assert a.category == "Snv"
            i = a.position - 1
            counts[i, codes[i], 0] -= a.support
            counts[i, _abi.ALLELE_OF_BASE[a.alt], 0] += a.support
    assert counts.min() >= 0
    return counts


def tile_starts(n):
    """First positions of the tiles the streaming surface cuts a chromosome of n bases into: 64 loci from every block's start."""
    return [s + k for s in range(1, n + 1, BLOCK) for k in range(0, BLOCK, TILE) if s + k <= n]


def observations_of(chrom, alleles, overhang=0):
    """(positions, tuples) for AddObservations / orc.run_observations, (stream, tiles) for pisces_hip_call_tiles with the streaming
    surface's tile geometry (the last tile of a block and of the chromosome ragged)."""
    counts = folded_counts(chrom, alleles, overhang)
    n = len(chrom) + overhang
    idx = np.nonzero(counts.reshape(-1))[0]
    reps = counts.reshape(-1)[idx]
    locus, code, direction = idx // 18, (idx // 3) % 6, idx % 3
    starts = np.array(tile_starts(n))
    ends = np.minimum(np.minimum(starts + TILE, ((starts - 1) // BLOCK + 1) * BLOCK + 1), n + 1)
    tile_of = np.searchsorted(starts, locus + 1, side="right") - 1
    in_tile = locus + 1 - starts[tile_of]
    assert (code < _abi.ALLELE_N).all()
    cell = _abi.tuple_pack(in_tile.astype(np.uint32), np.full(len(idx), ANCHOR, np.uint32), direction.astype(np.uint32), code.astype(np.uint32),
                           np.full(len(idx), 37, np.uint32)).astype(np.uint32)
    tuples = np.repeat(cell, reps)
    positions = np.repeat((locus + 1).astype(np.int32), reps)
    per_tile = np.bincount(np.repeat(tile_of, reps), minlength=len(starts))
    begin = 1 + np.concatenate([[0], np.cumsum(per_tile)[:-1]])
    tiles = np.zeros(len(starts), dtype=_abi.TILE_DTYPE)
    tiles["start_position"], tiles["n_loci"], tiles["tuple_begin"], tiles["tuple_end"] = starts, ends - starts, begin, begin + per_tile
    stream = np.concatenate([np.full(1, _abi.TUPLE_PAD, np.uint32), tuples, np.full(3, _abi.TUPLE_PAD, np.uint32)])
    return positions, tuples, stream, tiles


def reads_of(chrom, alleles, width=50):
    """A ReadBatch with the layout's counts: COV forward reads over every `width` bases, the alternate base of the k-th allele from counts in
    the first (k even) or last (k odd) `support` reads of its chunk, so that two neighbouring SNVs never share a read (no MNV is found).
    (Where the reference is N the reads are N: no coverage there, and no allele of an SNV layout either.)"""
    n = len(chrom)
    ref = np.frombuffer(chrom.encode(), np.uint8)
    pos, lens, bases = [], [], []
    snvs = sorted((a for a in alleles if a.from_counts), key=lambda a: a.position)
    for first in range(1, n + 1, width):
        w = min(width, n + 1 - first)
        rows = np.repeat(ref[None, first - 1:first - 1 + w], COV, axis=0).copy()
        for k, a in enumerate(snvs):
            if first <= a.position < first + w:
                assert a.support <= COV // 2 or a.support == COV
                who = slice(0, a.support) if k % 2 == 0 else slice(COV - a.support, COV)
                rows[who, a.position - first] = ord(a.alt)
        bases.append(rows.reshape(-1))
        pos.append(np.full(COV, first, np.int32))
        lens.append(np.full(COV, w, np.int64))
    lens = np.concatenate(lens)
    m = len(lens)
    allb = np.concatenate(bases)
    return _abi.ReadBatch.from_arrays(position=np.concatenate(pos), flags=np.zeros(m, np.uint8), cigar_offset=np.arange(m + 1, dtype=np.int32),
                                      cigar_op=np.full(m, ord("M"), np.uint8), cigar_len=lens.astype(np.uint32),
                                      seq_offset=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), bases=allb,
                                      quals=np.full(len(allb), 37, np.uint8))


def candidate_dicts(alleles):
    """The alleles that do not come from counts, as engine.AddCandidates takes them."""
    return [{"position": a.position, "category": CAT[a.category], "ref": a.ref, "alt": a.alt, "support_by_dir": (a.support, 0, 0),
             "well_anchored_by_dir": (a.support, 0, 0)} for a in alleles if not a.from_counts and not a.no_row]


def bits_of_rows(rows, allele_strings):
    """{key: (FILTER_RMXN bit, support, coverage)} of the variant rows of a run."""
    out = {}
    for r, (ref, alt) in zip(rows, allele_strings):
        cat = int(_abi.info_category(int(r["info"])))
        if cat == _abi.CAT_REFERENCE:
            continue
        k = (CAT_NAME[cat], int(r["position"]), ref, alt)
        assert k not in out, k
        out[k] = ((int(r["filter_bits"]) >> _abi.FILTER_RMXN) & 1, int(r["allele_support"]), int(r["total_coverage"]))
    return out


def oracle_run(chrom, alleles, cfg, overhang=0):
    """The layout through the oracle: the counts set into a state, every allele a candidate, AlleleCaller.Call (orc.call_candidates)."""
    n = len(chrom) + overhang
    st = orc.State(1, n + 16, min_bq=cfg.min_base_call_quality)   # (a deletion may reach past the last base: those loci have no counts)
    na = orc.lib.orc_num_anchor_indexes(st.h)
    a = np.ctypeslib.as_array(orc.lib.orc_counts_ptr(st.h), shape=(n + 16, 6, 3, na))
    a[:n, :, :, ANCHOR] = folded_counts(chrom, alleles, overhang)
    cands = [orc.make_candidate(x.position, CAT[x.category], x.ref, x.alt, support=(x.support, 0, 0), well_anchored=(x.support, 0, 0)) for x in alleles if not x.no_row]
    rows, full, _ = orc.call_candidates(st, cands, cfg, chrom.encode())
    return bits_of_rows(rows, [(f.ref.decode(), f.alt.decode()) for f in full])


def check(got, chrom, alleles, max_unit, min_rep, limit, where=""):
    """Every allele has its row, and the row's bit is the statement's for the row's own support and coverage.  Returns the expected bits."""
    missing = [key_of(a) for a in alleles if (key_of(a) not in got) != a.no_row]
    assert not missing, (where, missing[:5])
    exp = expected_bits(chrom, alleles, max_unit, min_rep, limit, {k: v[1:] for k, v in got.items()})
    wrong = [(k, got[k], exp[k]) for k in exp if got[k][0] != exp[k]]
    assert not wrong, (where, (max_unit, min_rep, limit), len(wrong), wrong[:8])
    return exp


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference's table
# ------------------------------------------------------------------------------------------------------------------------------------
def table():
    with open(os.path.join(G, "rmxn_cases.json")) as f:
        return json.load(f)


def table_settings(t, case):
    """[(max_unit, min_rep, limit, flagged)]: the five settings the harness puts a case's alleles under (six assertions, one twice)."""
    seen = []
    for a in t["assertions"]:
        s = (case["max_unit"], case["repeats"] + a["min_rep_delta"], a["frequency_limit"], a["flagged"])
        if s not in seen:
            seen.append(s)
    assert len(seen) == 5
    return seen


def table_alleles(case, offset=0):
    return [allele(x["category"], x["position"] + offset, x["ref"], x["alt"], support=COV // 5, name="line %d" % case["line"], from_counts=False)
            for x in case["alleles"]]


def joined_table(t):
    """One chromosome of all the table's sequences with an N between them (no variant base is N: no motif runs across a joint), an N in
    front and eight behind; [(case, its alleles on the joined chromosome)]."""
    chrom, out = "N", []
    for case in t["cases"]:
        assert "N" not in case["variant"]
        out.append((case, table_alleles(case, offset=len(chrom))))
        chrom += case["sequence"].replace("*", "") + "N"
    return chrom + "N" * 7, out


# ------------------------------------------------------------------------------------------------------------------------------------
# the directed SNV grid
# ------------------------------------------------------------------------------------------------------------------------------------
SNV_SETTINGS = [(5, m, LIMIT) for m in list(range(0, 13)) + [32, 33, 40]] + [(0, 0, LIMIT), (0, 1, LIMIT), (1, 0, LIMIT), (1, 9, LIMIT), (-1, 9, LIMIT),
                                                                             (5, 9, 1.0), (5, 9, 1.5)]
_FILL = "GTGATCTAGCATGCTACGTCAGTCGATGCATCAGT"   # no base twice in a row, no A or C run


def snv_grid():
    """(chromosome, alleles, built): every SNV is A>C; built: {name: (c1, i1, i2)} the run lengths each named case was built with — the
    reference-base run through the SNV, the alternate-base run behind it and the one in front of it."""
    chrom, alleles, built = [], [], {}
    state = SimpleNamespace(n=0, fill=0)

    def fill(k):
        for _ in range(k):
            chrom.append(_FILL[state.fill % len(_FILL)])
            state.fill += 1
            state.n += 1

    def locus_of(p):
        return ((p - 1) % BLOCK) % TILE

    def put(name, left, right, c1, i1, i2, locus=None, support=4):
        """G + left + [A] + right + G behind at least two filler bases; locus: where in a tile the SNV lands (None: wherever it comes)."""
        fill(2)
        while locus is not None and locus_of(state.n + len(left) + 2) != locus:
            fill(1)
        chrom.extend("G" + left + "A")
        state.n += len(left) + 2
        alleles.append(allele("Snv", state.n, "A", "C", support=support, name=name))
        chrom.extend(right + "G")
        state.n += len(right) + 1
        built[name] = (c1, i1, i2)

    # chromosome start: a run that begins at position 1, SNVs at positions 1, 2 and at the run's last base
    chrom.extend("A" * 10 + "C" * 9 + "G")
    state.n = 20
    for p, nm, b in ((1, "position 1", (10, 0, 0)), (2, "position 2", (10, 0, 0)), (10, "run from position 1", (10, 9, 0))):
        alleles.append(allele("Snv", p, "A", "C", name=nm))
        built[nm] = b
    # short repeats at tile edges
    for m in (2, 8, 9):
        for x in (m - 1, m, m + 1):
            for y in (m - 1, m, m + 1):
                for locus in (0, 63):
                    put("edge m%d ref%d alt%d behind, locus %d" % (m, x, y, locus), "A" * (x - 1), "C" * y, x, y, 0, locus)
                    put("edge m%d ref%d alt%d in front, locus %d" % (m, x, y, locus), "C" * y, "A" * (x - 1), x, 0, y, locus)
    # the eight-neighbour shortcut: reference-base runs of 0..5 on either side; an alternate run where one side is free
    for left in range(6):
        for right in range(6):
            if left == 0:
                put("near l0 r%d" % right, "C" * 12, "A" * right, 1 + right, 0, 12)
            elif right == 0:
                put("near l%d r0" % left, "A" * left, "C" * 12, 1 + left, 12, 0)
            else:
                put("near l%d r%d" % (left, right), "A" * left, "A" * right, 1 + left + right, 0, 0)
    # the margin: runs of 31..34 that end at the SNV and start behind it, at locus 0 and at locus 63
    for x in (31, 32, 33, 34):
        for y in (31, 32, 33, 34):
            for locus in (0, 63):
                put("margin ref%d alt%d behind, locus %d" % (x, y, locus), "A" * (x - 1), "C" * y, x, y, 0, locus)
                put("margin ref%d alt%d in front, locus %d" % (x, y, locus), "C" * y, "A" * (x - 1), x, 0, y, locus)
    put("homopolymer of 100 across two tile edges", "A" * 99, "C" * 45, 100, 45, 0, locus=40)
    # N
    put("run broken by one N", "AAAANAAAA", "C" * 9, 5, 9, 0)
    fill(2)
    chrom.extend("GN" + "C" * 9 + "G")
    alleles.append(allele("Snv", state.n + 2, "N", "C", name="reference base N beside a run of the alternate base", no_row=True))
    built[alleles[-1].name] = None
    state.n += 12
    # the limit: 7 of 20 is the limit 0.35f, 6 of 20 is below it, a homozygous alternate against 1.0 and beyond
    for s in (6, 7, COV):
        put("limit support %d" % s, "A" * 8, "C" * 9, 9, 9, 0, support=s)
    # chromosome end: a run that ends at the last base, SNVs at the last two bases and at the run's first; the last tile is ragged
    fill(3)
    while locus_of(state.n + 20) in (TILE - 1, (BLOCK - 1) % TILE) or locus_of(state.n + 20) < 2:   # a ragged last tile that holds the last two bases
        fill(1)
    chrom.extend("G" + "C" * 9 + "A" * 10)
    state.n += 20
    n = state.n
    for p, nm, b in ((n, "last base", (10, 0, 0)), (n - 1, "last base but one", (10, 0, 0)), (n - 9, "run to the last base", (10, 0, 9))):
        alleles.append(allele("Snv", p, "A", "C", name=nm))
        built[nm] = b
    return "".join(chrom), alleles, built


def snv_grid_holds(chrom, alleles, built):
    """On the statement: every named case has the run lengths it was built with, sits where its name says, and is decided as meant."""
    starts = tile_starts(len(chrom))
    assert 2 <= len(chrom) + 1 - starts[-1] < min(TILE, BLOCK % TILE), "the last tile is ragged"
    names = {a.name: a for a in alleles}
    assert len(names) == len(alleles) == len(built)
    over_n = [a for a in alleles if a.no_row]
    assert len(over_n) == 1 and chrom[over_n[0].position - 1:over_n[0].position + 9] == "N" + "C" * 9
    alleles = [a for a in alleles if not a.no_row]
    for a in alleles:
        c1, i1, i2 = built[a.name]
        assert chrom[a.position - 1] == a.ref == "A"
        assert rmxn_ref.length_for_indel(a.position - 1, "A", chrom, 5) == c1, a.name
        assert rmxn_ref.length_for_indel(a.position, "C", chrom, 5) == i1, a.name
        assert rmxn_ref.length_for_indel(a.position - 1, "C", chrom, 5) == i2, a.name
        if ", locus " in a.name:
            assert a.position - max(s for s in starts if s <= a.position) == int(a.name.rsplit(" ", 1)[1]), a.name
        for m in (0, 1, 2, 8, 9, 32, 33, 40):
            want = min(c1, max(i1, i2)) >= m and a.support * 20 < 7 * COV
            assert rmxn_ref.should_filter("Snv", a.position, "A", "C", chrom, 5, m, F32(LIMIT), a.support, COV) == want, (a.name, m)
    # the runs reach across the tile edge they were put at, and the margin runs fill or overflow the 32 staged bytes
    for a in alleles:
        if a.name.startswith(("edge", "margin")) and "ref1 " not in a.name:
            t = max(s for s in starts if s <= a.position)
            behind = "behind" in a.name
            if a.name.endswith("locus 0"):
                assert chrom[t - 2] == ("A" if behind else "C") and t == a.position and t > 1
            else:
                assert chrom[t + TILE - 1] == ("C" if behind else "A") and t + TILE in starts
    dec = lambda nm, m, lim=LIMIT: rmxn_ref.should_filter("Snv", names[nm].position, "A", "C", chrom, 5, m, F32(lim), names[nm].support, COV)
    assert dec("limit support 6", 9) and not dec("limit support 7", 9) and not dec("limit support %d" % COV, 9, 1.0) and dec("limit support %d" % COV, 9, 1.5)
    assert dec("margin ref32 alt32 behind, locus 63", 32) and not dec("margin ref32 alt32 behind, locus 63", 33) and not dec("margin ref31 alt34 behind, locus 0", 32)
    assert dec("margin ref34 alt33 in front, locus 0", 33) and not dec("margin ref34 alt33 in front, locus 0", 34)
    assert dec("homopolymer of 100 across two tile edges", 40) and not dec("run broken by one N", 9) and dec("run broken by one N", 5)
    assert dec("near l0 r3", 4) and not dec("near l0 r3", 5) and dec("near l4 r0", 5) and not dec("near l4 r0", 6) and not dec("near l2 r2", 1) and dec("near l2 r2", 0)
    assert dec("run from position 1", 9) and dec("run to the last base", 9) and not dec("position 1", 1) and dec("last base", 0)
    for m in (2, 8, 9):
        flagged = [a.name for a in alleles if a.name.startswith("edge m%d " % m) and dec(a.name, m)]
        assert len(flagged) == 4 * 4, (m, len(flagged))   # the combinations with both runs >= m, in four placements


# ------------------------------------------------------------------------------------------------------------------------------------
# the directed spanning grid
# ------------------------------------------------------------------------------------------------------------------------------------
SPAN_SETTINGS = [(u, m, 1.1) for u in (0, 1, 2, 5, 8) for m in (0, 1, 2, 3, 6, 9)] + [(5, 6, LIMIT), (5, 6, 0.1)]
_UNITS = {1: "T", 2: "AC", 3: "ACG", 4: "ACGT", 5: "ACGTA", 6: "ACGTAG"}
_TAIL35 = "GATCTAGCATGCTAGCTGACTCGATGCATCGTCAG"   # 35 bases, no unit of 1..5 twice in a row at either end


def spanning_grid():
    """(chromosome, alleles, built): built = {name: {max_unit: component 1}} for insertions and deletions ({max_unit: (c1, c2)} for MNVs)
    as the case was built; insertions and deletions and MNVs are candidates."""
    chrom, alleles, built = [], [], {}

    def pos():
        return len(chrom)

    def add(name, category, position, ref, alt, expect):
        alleles.append(allele(category, position, ref, alt, name=name, from_counts=False))
        built[name] = expect

    # start: an AC repeat from position 1 (the ratchet reaches index 0), an MNV at position 1
    chrom.extend("AC" * 6 + "GG" + "T")
    add("MNV at position 1", "Mnv", 1, "AC", "CA", {1: (1, 1), 2: (6, 1), 5: (6, 1)})
    add("ratchet to index 0, insertion", "Insertion", 8, "C", "CAC", {0: 0, 1: 1, 2: 6, 8: 6})
    add("ratchet to index 0, deletion", "Deletion", 8, "C", None, {0: 0, 1: 1, 2: 6, 8: 6})
    add("both ends repeat", "Insertion", 12, "C", "CACACGG", {1: 2, 2: 6, 5: 6})
    # unit lengths 1..6: six copies, an insertion of one more in front of them and a deletion of one inside
    for u, unit in _UNITS.items():
        chrom.extend("GA" if unit[0] != "A" else "GT")
        anchor = pos()
        chrom.extend(unit * 6 + ("C" if unit[-1] != "C" else "G"))
        whole = {m: (6 if m >= u else None) for m in (0, 1, 2, 5, 8)}
        add("unit %d, insertion" % u, "Insertion", anchor, chrom[anchor - 1], chrom[anchor - 1] + unit, whole)
        add("unit %d, deletion" % u, "Deletion", anchor + 2 * u, chrom[anchor + 2 * u - 1], None, whole)
    # a repeat only a prefix sees, only a suffix sees
    chrom.extend("TG")
    anchor = pos()
    chrom.extend("ACG" * 3 + "T")
    add("prefix only", "Insertion", anchor, "G", "G" + "ACGTT", {2: 1, 3: 3, 5: 3})
    add("suffix only", "Insertion", anchor + 9, "G", "G" + "TTACG", {2: 1, 3: 3, 5: 3})
    # 40 bases in the byte pool: the first five repeat behind the insertion, the last five in front of it
    chrom.extend("CG")
    anchor = pos()
    chrom.extend("ACGTA" * 9 + "C")
    add("insertion of 40, its first 5 repeat", "Insertion", anchor, "G", "G" + "ACGTA" + _TAIL35, {4: None, 5: 9, 8: 9})
    add("insertion of 40, its last 5 repeat", "Insertion", anchor + 45, "A", "A" + _TAIL35 + "ACGTA", {4: None, 5: 9, 8: 9})
    # end: a repeat that runs to the last base with a deletion inside, an MNV that ends on the last base
    chrom.extend("TGG" + "CA" * 6)
    n = pos()
    add("deletion inside a repeat to the last base", "Deletion", n - 6, "A", None, {1: 1, 2: 6, 5: 6})
    add("deletion of the last bases", "Deletion", n - 2, "A", None, {1: 1, 2: 6})
    add("MNV ending on the last base", "Mnv", n - 1, "CA", "AC", {1: (1, 1), 2: (6, 1)})
    add("insertion behind the last base", "Insertion", n, "A", "ACA", {1: 1, 2: 6})
    chrom = "".join(chrom)
    for a in alleles:   # a deletion takes the bases that stand there
        if a.alt is None:
            u = int(a.name.split()[1].rstrip(",")) if a.name.startswith("unit") else 2
            a.alt, a.ref = a.ref, chrom[a.position - 1:a.position + u]
    return chrom, alleles, built


def spanning_grid_holds(chrom, alleles, built):
    assert len({a.name for a in alleles}) == len(alleles) == len(built)
    for a in alleles:
        if a.category != "Insertion":
            assert chrom[a.position - 1:a.position - 1 + len(a.ref)] == a.ref, a.name
        else:
            assert chrom[a.position - 1] == a.ref == a.alt[0], a.name
        for max_unit, want in built[a.name].items():
            c1, c2 = rmxn_ref.component_lengths(a.category, a.position, a.ref, a.alt, chrom, max_unit)
            if want is None:
                assert c1 < 6, (a.name, max_unit, c1)
            elif a.category == "Mnv":
                assert (c1, c2) == want, (a.name, max_unit, c1, c2)
            else:
                assert c1 == want and c2 == rmxn_ref.INT_MAX, (a.name, max_unit, c1)
    by = {a.name: a for a in alleles}
    assert len(by["insertion of 40, its first 5 repeat"].alt) == 41 and by["MNV at position 1"].position == 1
    last = by["MNV ending on the last base"]
    assert last.position + len(last.ref) - 1 == len(chrom) and by["insertion behind the last base"].position == len(chrom)
    d = by["deletion of the last bases"]
    assert d.position + len(d.ref) - 1 == len(chrom)


# ------------------------------------------------------------------------------------------------------------------------------------
# the seeded generator
# ------------------------------------------------------------------------------------------------------------------------------------
def fuzz_layout(seed, n_alleles=250, length=3000, long_runs=True):
    """(chromosome, alleles): a reference of repeated units of 1-4 bases with single bases and N in between; alleles of all four
    categories, valid by construction (an SNV / MNV / deletion's reference allele is the chromosome's, first and last base of an MNV differ
    from the reference, no alternate base is N), most of them built from the bases next to them so that repeats are found; one of every
    category at position 1 and at the last base.  SNVs come from counts, no two alleles from counts within reach of one MNV, MNVs and SNVs
    apart."""
    rng = np.random.default_rng(seed)
    parts = []
    total = 0
    while total < length:
        u = int(rng.integers(1, 5))
        unit = "".join(rng.choice(list("ACGT"), u))
        k = int(rng.integers(1, 13))
        if long_runs and rng.random() < 0.06:
            k = int(rng.integers(30, 46)) if u == 1 else int(rng.integers(10, 20))
        seg = unit * k + ("N" if rng.random() < 0.1 else str(rng.choice(list("ACGT")))) * int(rng.integers(0, 2))
        parts.append(seg)
        total += len(seg)
    chrom = "".join(parts)[:length]
    chrom = chrom[:6].replace("N", "A") + chrom[6:-6].replace("NN", "NA") + chrom[-6:].replace("N", "C")   # (no N under the alleles at the ends)
    n = len(chrom)
    taken = np.zeros(n + 12, bool)    # positions an SNV or MNV holds, with the reach of an MNV around them
    alleles, keys = [], set()

    def other(b, near):
        for c in near:
            if c != b and c != "N":
                return c
        return str(rng.choice([c for c in "ACGT" if c != b]))

    def local(p, length_):
        """Bases for an inserted / alternate allele: what follows, what precedes, or random."""
        how = rng.integers(0, 4)
        s = chrom[p:p + length_] if how == 0 else chrom[max(0, p - length_):p] if how == 1 else (chrom[p:p + max(1, length_ // 2)] * length_)[:length_] if how == 2 else ""
        if len(s) != length_ or "N" in s:
            s = "".join(rng.choice(list("ACGT"), length_))
        return s

    def try_add(category, p, ln=None):
        if category == "Snv":
            if chrom[p - 1] == "N" or taken[max(0, p - 4):p + 4].any():
                return False
            a = allele("Snv", p, chrom[p - 1], other(chrom[p - 1], chrom[p:p + 1] + chrom[max(0, p - 2):p - 1]))
            lo, hi = p, p
        elif category == "Mnv":
            ln = ln or int(rng.integers(2, 6))
            if p + ln - 1 > n or "N" in chrom[p - 1:p - 1 + ln] or taken[max(0, p - 4):p + ln + 3].any():
                return False
            ref = chrom[p - 1:p - 1 + ln]
            alt = list(local(p + ln - 1 if rng.random() < 0.5 else p - 1, ln))
            alt[0], alt[-1] = other(ref[0], alt[0] + chrom[max(0, p - 2):p - 1]), other(ref[-1], alt[-1] + chrom[p + ln - 1:p + ln])
            a = allele("Mnv", p, ref, "".join(alt))
            lo, hi = p, p + ln - 1
        elif category == "Insertion":
            if chrom[p - 1] == "N":
                return False
            a = allele("Insertion", p, chrom[p - 1], chrom[p - 1] + local(p, ln or int(rng.choice([1, 1, 2, 2, 3, 4, 5, 6, 9]))))
            lo = hi = None
        else:
            ln = ln or int(rng.choice([1, 1, 2, 2, 3, 4, 5, 6, 9]))
            if p + ln > n or chrom[p - 1] == "N" or "N" in chrom[p:p + ln]:
                return False
            a = allele("Deletion", p, chrom[p - 1:p + ln], chrom[p - 1])
            lo = hi = None
        if key_of(a) in keys:
            return False
        a.support = int(rng.choice([4, 4, 4, 6, 7, 8]))
        keys.add(key_of(a))
        alleles.append(a)
        if lo is not None:
            taken[lo - 1:hi] = True
        return True

    # the chromosome's two ends: an insertion and a deletion at both, an SNV at one and an MNV at the other (the two would share loci)
    first, last = ("Snv", "Mnv") if seed % 2 == 0 else ("Mnv", "Snv")
    assert try_add(first, 1, 2) and try_add("Insertion", 1, 2) and try_add("Deletion", 1, 2)
    assert try_add(last, n - 1 if last == "Mnv" else n, 2) and try_add("Insertion", n, 2) and try_add("Deletion", n - 2, 2)
    cats = ["Snv", "Mnv", "Insertion", "Deletion"]
    while len(alleles) < n_alleles:
        try_add(cats[int(rng.integers(0, 4))], int(rng.integers(1, n + 1)))
    for a in alleles:
        a.name = "seed %d %s %d %s>%s" % (seed, a.category, a.position, a.ref, a.alt)
    return chrom, alleles


def at_an_end(a, n):
    return a.position == 1 or a.position + len(a.ref) - 1 == n


def fuzz_is_not_vacuous(cases):
    """cases: [(allele, chromosome length, max_unit, flagged)] over every layout and setting of a fuzz."""
    flagged = sum(1 for c in cases if c[3])
    assert 0.15 * len(cases) <= flagged <= 0.60 * len(cases), (flagged, len(cases))
    for want in (0, 1):
        some = [c for c in cases if c[3] == want]
        assert {c[0].category for c in some} == set(CAT), want
        units = {c[2] for c in some}
        assert min(units) == 0 and max(units) == 8, (want, units)
        assert any(c[0].position == 1 for c in some) and any(c[0].position + len(c[0].ref) - 1 == c[1] for c in some), want
    return flagged


FUZZ_SEEDS = (11, 12, 13)


def fuzz_settings(seed, repetitions=tuple(range(10))):
    """Twelve (max_unit, min_rep, limit) of a seed: both unit-length extremes with a repetition count that flags and one that does not, then
    draws from unit lengths 0..8 and the given repetitions; limits at (7 of 20 is 0.35f), just under and just above a frequency the
    alleles have, and out of every allele's reach."""
    rng = np.random.default_rng(1000 + seed)
    at = np.float32(LIMIT)
    limits = [float(at), float(np.nextafter(at, np.float32(0))), float(np.nextafter(at, np.float32(1))), 1.0, 1.1]
    assert rmxn_ref.frequency(7, 20) == at
    fixed = [(0, 0), (0, 1), (8, 1), (8, int(max(repetitions)))]
    drawn = [(int(rng.integers(0, 9)), int(rng.choice(repetitions))) for _ in range(8)]
    return [(u, m, limits[int(rng.integers(0, len(limits)))]) for u, m in fixed + drawn]


NOT_FROM_READS = ("insertion behind the last base", "deletion of the last bases")   # no read shows an allele with nothing aligned behind it


def spanning_reads(chrom, alleles, flank=15):
    """(ReadBatch, the alleles in it): the spanning grid as reads — COV forward reads of the reference over every 50 bases, and for every
    allele a read can show four reads with it in their CIGAR / bases, `flank` aligned bases (or what the chromosome has) on either side."""
    n = len(chrom)
    shown = [a for a in alleles if a.name not in NOT_FROM_READS]
    reads = []
    for first in range(1, n + 1, 50):
        w = min(50, n + 1 - first)
        reads += [{"pos": first, "cigar": [("M", w)], "seq": chrom[first - 1:first - 1 + w].encode(), "quals": [37] * w, "reverse": False}] * COV
    for a in shown:
        start = max(1, a.position - flank)
        if a.category == "Mnv":
            end = min(n, a.position + len(a.ref) - 1 + flank)
            seq = chrom[start - 1:a.position - 1] + a.alt + chrom[a.position - 1 + len(a.ref):end]
            cigar = [("M", len(seq))]
        elif a.category == "Insertion":
            end = min(n, a.position + flank)
            seq = chrom[start - 1:a.position] + a.alt[1:] + chrom[a.position:end]
            cigar = [("M", a.position - start + 1), ("I", len(a.alt) - 1), ("M", end - a.position)]
        else:
            gone = len(a.ref) - 1
            end = min(n, a.position + gone + flank)
            seq = chrom[start - 1:a.position] + chrom[a.position + gone:end]
            cigar = [("M", a.position - start + 1), ("D", gone), ("M", end - a.position - gone)]
        assert all(l > 0 for _, l in cigar), a.name
        reads += [{"pos": start, "cigar": cigar, "seq": seq.encode(), "quals": [37] * len(seq), "reverse": False}] * a.support
    reads.sort(key=lambda r: r["pos"])
    return _abi.ReadBatch(reads), shown
