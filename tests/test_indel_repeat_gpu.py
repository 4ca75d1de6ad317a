"""FilterType.IndelRepeatLength on the device: indel_repeat_kernel behind call_spanning_kernel, on every route a flush's rows take, beside
the other modes, and the R<n> name in the device formatter.  The checker is the plain-Python statement of
AlleleProcessor.ComputeIndelRepeatLength (tests/indel_repeat_ref.py), fed every row's own alleles; a handle without the filter gives what
the rest of every row must be.

The scenario: a chromosome of about 300 bases — plain sequence, G + A x 9 (the run's fourth base at position 100, so that a deletion
anchored there lies across the edge of blocks of 100), plain sequence, G + ATC x 8, plain sequence, G + T x 10 to the last base — and about
40 reads of 60 bases over every stretch, plus 40 per planted allele.
"""
import numpy as np
import pytest

from pisces_amd import _abi
from tests import indel_repeat_ref as ref
from tests.test_read_store import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
BIT = 1 << _abi.FILTER_INDEL_REPEAT_LENGTH
FORCED = 1 << _abi.FILTER_FORCED_REPORT
CAT_NAME = {_abi.CAT_SNV: "Snv", _abi.CAT_INSERTION: "Insertion", _abi.CAT_DELETION: "Deletion", _abi.CAT_MNV: "Mnv", _abi.CAT_REFERENCE: "Reference"}
_FILL = "GTGATCTAGCATGCTACGTCAGTCGATGCATCAGT"   # no base twice in a row
READS_PER_ALLELE = 40


def _build():
    fill = lambda k, at=0: "".join(_FILL[(at + i) % len(_FILL)] for i in range(k))
    chrom = fill(96) + "G" + "A" * 9 + "C"
    a0 = 97                                    # the G in front of the A run: the run is a0 + 1 .. a0 + 9
    assert chrom[a0 - 1] == "G" and chrom[a0:a0 + 9] == "A" * 9 and len(chrom) == a0 + 10
    chrom += fill(43, 3) + "G"
    b0 = len(chrom)                            # the G in front of the ATC run
    chrom += "ATC" * 8 + "G"
    p0 = len(chrom)                            # plain sequence from p0 + 1
    chrom += fill(80, 7) + "G" + "T" * 10
    n = len(chrom)
    plain_ins, plain_del, = p0 + 20, p0 + 45
    alleles = {
        "insertion of A in front of the A run": ("Insertion", a0, "G", "GA"),
        "deletion of A inside the A run, across position 100 | 101": ("Deletion", a0 + 3, "AA", "A"),
        "insertion of AA inside the A run": ("Insertion", a0 + 5, "A", "AAA"),
        "insertion of ATC in front of its run": ("Insertion", b0, "G", "GATC"),
        "insertion in plain sequence": ("Insertion", plain_ins, chrom[plain_ins - 1], chrom[plain_ins - 1] + "CA"),
        "deletion in plain sequence": ("Deletion", plain_del, chrom[plain_del - 1:plain_del + 2], chrom[plain_del - 1]),
        "SNV inside the A run": ("Snv", a0 + 2, "A", "C"),
        "MNV inside the A run": ("Mnv", a0 + 7, "AA", "CG"),
        "insertion on the second-to-last base, inside a homopolymer": ("Insertion", n - 1, "T", "TT"),
    }
    assert alleles["deletion of A inside the A run, across position 100 | 101"][1] == 100
    return chrom, alleles, dict(a0=a0, b0=b0, p0=p0)


CHROM, ALLELES, AT = _build()
N = len(CHROM)


def _read(start, cigar, seq, k):
    return {"pos": start, "cigar": cigar, "seq": seq.encode(), "quals": [37] * len(seq), "reverse": bool(k & 1)}


def scenario_reads(flank=30):
    """READS_PER_ALLELE reference reads over every 60 bases (every other one reverse), and for every planted allele as many reads that show
    it with `flank` aligned bases on either side, or what the chromosome has; the reads of the last insertion end ...1I1M."""
    reads = []
    for first in range(1, N + 1, 60):
        w = min(60, N + 1 - first)
        reads += [_read(first, [("M", w)], CHROM[first - 1:first - 1 + w], k) for k in range(READS_PER_ALLELE)]
    for name, (category, p, r, a) in ALLELES.items():
        start = max(1, p - flank + 1)
        if category in ("Snv", "Mnv"):
            end = min(N, p + len(r) - 1 + flank)
            seq = CHROM[start - 1:p - 1] + a + CHROM[p - 1 + len(r):end]
            cigar = [("M", len(seq))]
        elif category == "Insertion":
            end = min(N, p + flank)
            seq = CHROM[start - 1:p] + a[1:] + CHROM[p:end]
            cigar = [("M", p - start + 1), ("I", len(a) - 1), ("M", end - p)]
        else:
            gone = len(r) - 1
            end = min(N, p + gone + flank)
            seq = CHROM[start - 1:p] + CHROM[p + gone:end]
            cigar = [("M", p - start + 1), ("D", gone), ("M", end - p - gone)]
        assert all(l > 0 for _, l in cigar), name
        reads += [_read(start, cigar, seq, k) for k in range(READS_PER_ALLELE)]
    assert reads[-1]["cigar"][-2:] == [("I", 1), ("M", 1)] and reads[-1]["pos"] + 30 == N
    reads.sort(key=lambda x: x["pos"])
    return reads


def config(**kw):
    base = dict(collapse=0, call_mnvs=1, max_mnv_length=3, max_gap_between_mnv=1)
    base.update(kw)
    return _abi.default_config(**base)


def batch():
    return _abi.ReadBatch([dict(r) for r in scenario_reads()])


def run(cfg, threshold, route="flush_ex", setup=None, add=None):
    """One handle, the scenario's reads, one flush by `route`: (rows, allele strings or None)."""
    from pisces_amd import engine
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(CHROM)
        if setup:
            setup(c)
        if threshold is not None:
            c.SetIndelRepeatFilter(threshold)
        if route == "device reads + view":
            c.AddDeviceReads(engine.DeviceReadBatch.from_host(batch(), "cuda:0"))
        else:
            c.AddAlleleCounts(batch())
        if add:
            add(c)
        if route == "flush_ex":
            return c.CallWithAlleles()
        if route == "flush":
            return c.Call(), None
        if route == "device reads + view":
            return np.array(c.CallView(), copy=True), None
        if route == "begin / end":
            c.CallBegin()
            return c.CallEnd(), None
        if route == "begin / end_ex":
            c.CallBegin()
            return c.CallEndWithAlleles()
        if route == "a buffer too small first":
            return c.Call(capacity=4), None
        if route == "two flushes":
            first, first_alleles = c.CallWithAlleles(150)
            second, second_alleles = c.CallWithAlleles()
            assert len(first) and len(second) and int(first["position"].max()) <= 100 < int(second["position"].min())
            return np.concatenate([first, second]), first_alleles + second_alleles
        raise AssertionError(route)


def stated(rows, alleles, threshold):
    """The statement's answer for every row, from the row's own category, position and alleles."""
    return [ref.is_flagged(threshold, CAT_NAME[int(_abi.info_category(int(r["info"])))], int(r["position"]), a[0], a[1], CHROM) for r, a in zip(rows, alleles)]


def keys_of(rows, alleles):
    return [(CAT_NAME[int(_abi.info_category(int(r["info"])))], int(r["position"]), a[0], a[1]) for r, a in zip(rows, alleles)]


def hold(plain, plain_alleles, got, got_alleles, threshold, where):
    """The filtering handle's rows are the plain handle's except bit 7, and bit 7 is the statement's.  Returns the statement's answers."""
    assert got_alleles == plain_alleles and len(got) == len(plain), where
    assert not (plain["filter_bits"] & BIT).any(), where
    masked = got.copy()
    masked["filter_bits"] &= np.uint16(~BIT & 0xFFFF)
    assert masked.tobytes() == plain.tobytes(), where
    want = stated(got, got_alleles, threshold)
    have = [bool(int(r["filter_bits"]) & BIT) for r in got]
    wrong = [(k, h, w) for k, h, w in zip(keys_of(got, got_alleles), have, want) if h != w]
    assert not wrong, (where, wrong)
    return want


_PLAIN = {}


def plain_rows(call_mnvs=1):
    if call_mnvs not in _PLAIN:
        _PLAIN[call_mnvs] = run(config(call_mnvs=call_mnvs), None)
    return _PLAIN[call_mnvs]


def test_the_scenario_on_the_statement():
    """What the planted alleles are, on the statement alone (no device): lengths, and which side of 8 and of 2 each lies on."""
    length = {name: ref.indel_repeat_length(c, p, r, a, CHROM) for name, (c, p, r, a) in ALLELES.items()}
    assert length == {"insertion of A in front of the A run": 9, "deletion of A inside the A run, across position 100 | 101": 9,
                      "insertion of AA inside the A run": 9, "insertion of ATC in front of its run": 8, "insertion in plain sequence": 0,
                      "deletion in plain sequence": 1, "SNV inside the A run": 0, "MNV inside the A run": 0,
                      "insertion on the second-to-last base, inside a homopolymer": 1}, length
    for (c, p, r, a) in ALLELES.values():
        if c != "Insertion":
            assert CHROM[p - 1:p - 1 + len(r)] == r
        else:
            assert CHROM[p - 1] == r == a[0]
    assert 250 <= N <= 350 and CHROM[-11:] == "G" + "T" * 10


@pytest.mark.parametrize("call_mnvs", [1, 0], ids=["mnv calling on", "mnv calling off"])
def test_the_bit_against_the_statement(torch_cuda, call_mnvs):
    plain, plain_alleles = plain_rows(call_mnvs)
    keys = keys_of(plain, plain_alleles)
    planted = [v for v in ALLELES.values() if v[0] != "Mnv" or call_mnvs]
    assert all(v in keys for v in planted), [v for v in planted if v not in keys]
    cfg = config(call_mnvs=call_mnvs)
    for threshold in (8, 2):
        got, got_alleles = run(cfg, threshold)
        want = hold(plain, plain_alleles, got, got_alleles, threshold, threshold)
        spanning = [(k, w) for k, w in zip(keys, want) if k[0] in ("Insertion", "Deletion")]
        flagged = [k for k, w in spanning if w]
        cleared = [k for k, w in spanning if not w]
        if threshold == 8:
            assert len(flagged) >= 3 and len(cleared) >= 3, (flagged, cleared)
        assert ALLELES["insertion on the second-to-last base, inside a homopolymer"] in cleared
        assert ALLELES["deletion of A inside the A run, across position 100 | 101"] in flagged
        assert not any(w for k, w in zip(keys, want) if k[0] in ("Snv", "Mnv", "Reference"))
    off, off_alleles = run(cfg, 0)
    assert off_alleles == plain_alleles and off.tobytes() == plain.tobytes()


@pytest.mark.parametrize("route", ["flush", "device reads + view", "begin / end", "begin / end_ex", "a buffer too small first"])
def test_the_same_rows_through_every_route(torch_cuda, route):
    want, want_alleles = run(config(), 8)
    assert (want["filter_bits"] & BIT).sum() >= 3
    got, got_alleles = run(config(), 8, route=route)
    assert got.tobytes() == want.tobytes(), route
    assert got_alleles is None or got_alleles == want_alleles


def test_a_flagged_deletion_across_the_edge_of_two_flushes(torch_cuda):
    """Blocks of 100, a flush up to 150 (block 1, whose deletion at 100 ends in block 2) and the final one."""
    cfg = config(block_size=100)
    plain, plain_alleles = run(cfg, None, route="two flushes")
    got, got_alleles = run(cfg, 8, route="two flushes")
    want = hold(plain, plain_alleles, got, got_alleles, 8, "two flushes")
    keys = keys_of(got, got_alleles)
    i = keys.index(ALLELES["deletion of A inside the A run, across position 100 | 101"])
    assert want[i] and int(got[i]["filter_bits"]) & BIT
    assert sum(want) >= 3
    once, once_alleles = run(cfg, 8)
    assert sorted(keys_of(once, once_alleles)) == sorted(keys)


FORCED_ALLELE = (AT["a0"] + 1, "A", "AA")
ADDED = {"position": AT["b0"] + 3, "category": _abi.CAT_DELETION, "ref": "CATC", "alt": "C", "support_by_dir": (12, 12, 0), "well_anchored_by_dir": (12, 12, 0)}
# The per-locus genotypers: the ATC insertion is the one variant of its position and has half of the reads there (40 of 80), above MajorVF as
# set here, so the diploid models report it; the alleles of the A run share their coverage (40 of 240 each) and are the model's to keep or prune.
# (The haploid model prunes every variant beside which the reference keeps MinorVF of the reads, HaploidGenotyper.cs:36-83: none of this
# scenario's insertions or deletions would be left to look at.)
_VF = dict(diploid_snv_params=(0.10, 0.30, 0.80), diploid_indel_params=(0.10, 0.30, 0.80))
MODES = {
    "DiploidByThresholding": dict(cfg=dict(ploidy=_abi.PLOIDY_DIPLOID, call_mnvs=0, **_VF)),
    "DiploidByAdaptiveGT": dict(cfg=dict(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE, call_mnvs=0, min_frequency=0.0)),
    "the collapser on": dict(cfg=dict(collapse=1)),
    "CoverageMethod.Exact": dict(cfg=dict(), setup=lambda c: c.SetCoverageMethod("exact")),
    "a forced insertion without support": dict(cfg=dict(call_mnvs=0), setup=lambda c: c.SetForcedAlleles([FORCED_ALLELE])),
    "a candidate of pisces_hip_add_candidates": dict(cfg=dict(), add=lambda c: c.AddCandidates([ADDED])),
    "the amplicon filter on": dict(cfg=dict(call_mnvs=0), setup=lambda c: c.SetAmpliconBiasFilter(0.01)),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_other_modes_beside_it(torch_cuda, mode):
    m = MODES[mode]
    cfg = config(**m["cfg"])
    plain, plain_alleles = run(cfg, None, setup=m.get("setup"), add=m.get("add"))
    got, got_alleles = run(cfg, 8, setup=m.get("setup"), add=m.get("add"))
    want = hold(plain, plain_alleles, got, got_alleles, 8, mode)
    keys = keys_of(got, got_alleles)
    atc = keys.index(ALLELES["insertion of ATC in front of its run"])
    assert want[atc] and int(got[atc]["filter_bits"]) & BIT and want.count(False) >= 3, mode
    if "ploidy" not in m["cfg"]:
        assert sum(want) >= 3, mode   # (somatic: every planted allele is a row)
    if mode.startswith("a forced"):
        i = keys.index(("Insertion",) + FORCED_ALLELE)
        assert int(got[i]["allele_support"]) == 0 and int(got[i]["filter_bits"]) & FORCED and int(got[i]["filter_bits"]) & BIT
        assert ref.indel_repeat_length("Insertion", *FORCED_ALLELE, CHROM) == 9
    if mode.startswith("a candidate"):
        i = keys.index(("Deletion", ADDED["position"], "CATC", "C"))
        assert int(got[i]["filter_bits"]) & BIT and ref.indel_repeat_length("Deletion", ADDED["position"], "CATC", "C", CHROM) == 8
        assert CHROM[ADDED["position"] - 1:ADDED["position"] + 3] == "CATC"


def test_the_setter(torch_cuda):
    from pisces_amd import engine
    plain, plain_alleles = plain_rows(1)
    with engine.HipVariantCaller(config()) as c:
        c.SetReference(CHROM)
        with pytest.raises(engine.PiscesHipError) as e:
            c.SetIndelRepeatFilter(-1)
        assert e.value.code == _abi.E_INVALID_ARG
        c.AddAlleleCounts(batch())
        c.SetIndelRepeatFilter(8)   # any time: it holds from the next flush
        with pytest.raises(engine.PiscesHipError):
            c.SetIndelRepeatFilter(-8)   # refused: the threshold stays 8
        got, got_alleles = c.CallWithAlleles()
    assert sum(hold(plain, plain_alleles, got, got_alleles, 8, "set after the reads")) >= 3
    with engine.HipVariantCaller(config()) as c:
        c.SetReference(CHROM)
        c.SetIndelRepeatFilter(8)
        c.SetIndelRepeatFilter(0)   # off again
        c.AddAlleleCounts(batch())
        again, again_alleles = c.CallWithAlleles()
    assert again_alleles == plain_alleles and again.tobytes() == plain.tobytes()


def test_the_device_formatter_names_the_filter(torch_cuda):
    from pisces_amd import engine
    from tests.test_vcf_device_gpu import device_text, host_text
    rows, alleles = run(config(), 8)
    assert (rows["filter_bits"] & BIT).sum() >= 3
    kw = dict(noise_level_from_records=1)
    with engine.HipVariantCaller(_abi.default_config()) as c:
        want = host_text("chr7", rows, alleles=alleles, indel_repeat_filter=8, **kw)
        assert device_text(torch_cuda, c, "chr7", rows, alleles=alleles, indel_repeat_filter=8, **kw) == want
        assert sum(b"R8" in line.split(b"\t")[6].split(b";") for line in want.rstrip(b"\n").split(b"\n")) == int(((rows["filter_bits"] & BIT) != 0).sum())
        # threshold null: today's bytes — the text of the rows without the bit
        without = rows.copy()
        without["filter_bits"] &= np.uint16(~BIT & 0xFFFF)
        today = host_text("chr7", without, alleles=alleles, **kw)
        assert device_text(torch_cuda, c, "chr7", rows, alleles=alleles, **kw) == today == host_text("chr7", rows, alleles=alleles, **kw)
        assert device_text(torch_cuda, c, "chr7", rows, alleles=alleles, indel_repeat_filter=10, **kw) == host_text("chr7", rows, alleles=alleles, indel_repeat_filter=10, **kw)
