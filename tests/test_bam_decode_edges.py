"""The device BAM decode (pisces_hip_bam_decode + pisces_hip_add_decoded_reads: bam_kernels.hip.h, surface_bam.inc.h) past one pass of
its scans and at every record shape.  The streams come from tests/bam_synth.py, a writer that also says what the decode must make of
them; the CPU tests at the head of this file hold that writer to the plain reader of tests/golden/extract_bam_fixture.py and pin the
structure the large cases rely on.

  a. chunk counts 257 / 1024 / 1025 / 2049 (a second workgroup of the entry kernels; one, and two, carries of the single-workgroup
     scans) with zero-kept chunks across the pass edges, and stream lengths around the 32 KiB chunk;
  b. every nibble, sequence lengths around the 64-lane loop, every CIGAR op code, qualities, names, auxiliary fields;
  c. AlignmentSource.ShouldSkipRead as a truth table;
  d. the per-read refusals of the add, the lowest read winning, and what bam_decode itself refuses;
  e. any-CIGAR parity of the decoded add with the host-fed add.

bam_decode_kernel also writes op_quality / read_quality; nothing in the library reads them, so nothing here can check them.

Each group was seen to fail against a library with one line of bam_kernels.hip.h changed (on an MI355X, the repository untouched):
  the scans' results without base[] (bam_scan3_kernel)      test_chunk_counts... fails at 1025 and 2049 chunks, passes at 257 and 1024
  'A' and 'C' swapped in the nibble constants                test_every_record_shape_is_decoded_and_added fails
  bam_keep without its only_proper_pairs line                test_should_skip_read_truth_table fails
  first_error stored instead of atomicMin                    test_of_two_defective_reads_the_lower_index_is_named fails, all three cases
Measured there, host-side generation included: 2049 chunks (67 MB, the only two-carry case) 0.7 s, 1025 chunks 0.4 s, the decoded add at
1025 chunks 0.2 s a read path, any-CIGAR parity 2.0 s with MNV calling and 0.2 s without, every other case under 0.25 s."""
import functools
import struct

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import bam_synth as bs
from tests.test_bgzf import _bam_reads_reference, _kept, _string_tag, _expected_directions
from tests.test_read_store import env, oracle_counts, random_reads

ARRAYS = ("position", "flags", "cigar_offset", "cigar_op", "cigar_len", "seq_offset", "bases", "quals")


# ---------------------------------------------------------------- the cases (shared by the CPU and the GPU tests)
def _kept_pp(reads, chrom, min_mapq=1, skip_dups=True, proper=False):
    """_kept with ShouldSkipRead's proper-pair term (OnlyUseProperPairs && !IsProperPair, AlignmentsSource.cs:84-92)"""
    return [r for r in _kept(reads, chrom, min_mapq, skip_dups) if not proper or (r["flag"] & 0x2)]


def _batch_of_plain_reader(keep):
    """The PiscesReadBatch arrays of reads the plain reader parsed."""
    ops = [(ord(o), l) for r in keep for o, l in r["cigar"]]
    return dict(position=np.array([r["pos"] for r in keep], np.int64).astype(np.int32), flags=np.array([1 if r["flag"] & 0x10 else 0 for r in keep], np.uint8),
                cigar_offset=np.cumsum([0] + [len(r["cigar"]) for r in keep]).astype(np.int32), cigar_op=np.array([o for o, _ in ops], np.uint8),
                cigar_len=np.array([l for _, l in ops], np.uint32), seq_offset=np.cumsum([0] + [len(r["seq"]) for r in keep]).astype(np.int32),
                bases=np.frombuffer("".join(r["seq"] for r in keep).encode(), np.uint8), quals=np.frombuffer(b"".join(r["qual"].tobytes() for r in keep), np.uint8))


def _same_batch(got, want, what=""):
    for k in ARRAYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _writer_agrees_with_plain_reader(bam, filters):
    refs, reads = _bam_reads_reference(bam.file(1))
    assert refs == [n for n, _ in bam.refs] and len(reads) == bam.n_records
    for ref_id, mq, dups, proper in filters:
        want = bam.expected(ref_id, mq, dups, proper)
        keep = _kept_pp(reads, refs[ref_id], mq, dups, proper)
        assert want["reads"] == len(keep) and want["reads"] + want["skipped"] == sum(1 for r in reads if r["ref"] == refs[ref_id])
        _same_batch(_batch_of_plain_reader(keep), want["arrays"], f"filter {ref_id, mq, dups, proper}")
        if want["directions"] is not None:
            dirs, dd = _expected_directions(keep)
            np.testing.assert_array_equal(want["directions"], dirs)
            np.testing.assert_array_equal(want["deletion_directions"], dd)
        else:
            assert not any(_string_tag(r["tags"], b"XD") for r in keep)


# ---- 2b
SEQ_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)
QUAL_CYCLE = np.array([0, 41, 93, 254, 255], np.uint8)
SHAPE_REFS = (("chr1", 1_000_000), ("decode_only", 1_000_000))


def _shape_cigars(l):
    out = [[("M", l)]]
    if l >= 5:
        out.append([("H", 2), ("S", 1), ("M", l - 2), ("S", 1), ("H", 3)])
    if l >= 63:
        out.append([("S", 3), ("M", 10), ("I", 2), ("M", 5), ("D", 3), ("=", 8), ("X", 1), ("M", 4), ("P", 2), ("N", 6), ("M", l - 35), ("S", 2)])
    return out


@functools.lru_cache(maxsize=None)
def shapes_bam():
    """About two thousand records.  chr1: well-formed reads of every sequence length / CIGAR / quality / name / strand / auxiliary
    variant, every nibble at even and odd base indexes (bases the 4-bit table names, whatever the caller makes of them).  decode_only:
    shapes only the decode is asked about (no bases at all, reserved CIGAR op codes, a skip of 2^28 - 1).  One record of each
    (length, CIGAR) shape is then placed across a chunk boundary, the boundary falling in another of its fields every time."""
    w = bs.BamWriter(SHAPE_REFS)
    every = bs.aux_of_every_type()
    state = {"i": 0}

    def one(l, cig, v, ref_id=0, **kw):
        i = state["i"]
        state["i"] += 1
        nib = (np.arange(l) + v + (np.arange(l) // 16)) % 16            # every code at even and at odd indexes from l >= 33 on; v shifts it
        quals = np.full(l, 255, np.uint8) if v % 6 == 5 else QUAL_CYCLE[(np.arange(l) + v) % 5]   # (all 0xFF: the "missing" string)
        span = sum(n for _, n in cig) if ref_id == 0 else 0      # the expanded CIGAR: every operation takes its length
        aux = [dict(), dict(aux=every, xd=bs.xd_of_runs([(span // 3, "F"), (span // 3, "S"), (span - 2 * (span // 3), "R")]) if span >= 3 else "1F", aux_after=every),
               dict(aux=every), dict(xd=bs.xd_of_runs([(max(span - 1, 1), "R")]))][v % 4 if ref_id == 0 else 0]
        w.block([100 + 3 * i], cig, quals, nibbles=nib.astype(np.uint8), ref_id=ref_id, reverse=bool(v & 1), mapq=60,
                name=b"" if v % 3 == 0 else b"n" * 254 if v % 3 == 1 else b"read%05d" % i, **dict(aux, **kw))

    only = [(0, [("H", 3)], 0), (0, [("D", 2)], 1), (1, [("M", 1)], 5)] + [(10, [("M", 5), (op, 3), ("M", 5)], op) for op in range(9, 16)] + \
        [(30, [(op, 2 + op) for op in range(16)], 2), (10, [("M", 5), ("N", 2 ** 28 - 1), ("M", 5)], 4)]

    def decode_only(first):
        for l, cig, v in only[first:] + only[:first]:
            one(l, cig, v, ref_id=1)

    for l in SEQ_LENGTHS:
        for cig in _shape_cigars(l):
            for v in range(48):
                one(l, cig, v)
    decode_only(0)
    shapes = [(l, cig) for l in SEQ_LENGTHS for cig in _shape_cigars(l)]
    for j, (l, cig) in enumerate(shapes):
        v = 12 * (j % 4) + 1                                     # (variants 1 / 13 / 25 / 37: long name, every auxiliary type around the XD tag)
        size = 36 + 255 + 4 * len(cig) + (l + 1) // 2 + l + 2 * len(every) + 16
        inside = 1 + (j * 97) % (size - 40)                      # bytes of the record in front of the boundary
        gap = (-(w.offset + inside)) % bs.CHUNK
        w.filler(gap if gap >= 48 else gap + bs.CHUNK, 100 + 3 * state["i"])
        before = w.offset
        one(l, cig, v)
        assert before // bs.CHUNK != (w.offset - 1) // bs.CHUNK, "the record was to lie across a chunk boundary"
    for k in range(len(only)):                                   # each decode-only shape across a boundary as well
        gap = (-(w.offset + 20 + k)) % bs.CHUNK
        w.filler(gap if gap >= 48 else gap + bs.CHUNK, 100 + 3 * state["i"])
        decode_only(k)
    return w.finish()


# ---- 2c
FLAG_BITS = (0x2, 0x4, 0x10, 0x100, 0x400, 0x800)
FILTER_FLAGS = [0] + list(FLAG_BITS) + [a | b for i, a in enumerate(FLAG_BITS) for b in FLAG_BITS[i + 1:]]
FILTER_MAPQ = (0, 1, 19, 20, 21, 254, 255)
FILTER_REFS = (("chr1", 1_000_000), ("chr2", 1_000_000), ("chr3", 1_000_000), ("chr4", 1_000_000))
FILTER_SETTINGS = [(ref_id, mq, dups, proper) for ref_id in (0, 3) for mq in (0, 1, 20, 255) for dups in (False, True) for proper in (False, True)]


@functools.lru_cache(maxsize=None)
def filter_bam():
    """flag in {none, each of 0x2 0x4 0x10 0x100 0x400 0x800, every pair} x mapq x n_cigar_op in {0, 1} x ref_id in {-1, 0, 1, n_ref - 1}:
    1232 records, every one with bases and a position of its own."""
    rng = np.random.default_rng(2)
    grid = np.array([(f, q, nc, r) for r in (-1, 0, 1, 3) for nc in (0, 1) for q in FILTER_MAPQ for f in FILTER_FLAGS], np.int64)
    grid = grid[rng.permutation(len(grid))]
    assert len(grid) == 22 * 7 * 2 * 4
    w = bs.BamWriter(FILTER_REFS)
    for nc in (0, 1):
        i = np.flatnonzero(grid[:, 2] == nc)
        w.block(1000 + i, [("M", 10)] * nc, rng.integers(2, 42, (len(i), 10)), nibbles=rng.choice(np.array([1, 2, 4, 8], np.uint8), (len(i), 10)),
                ref_id=grid[i, 3], flag=grid[i, 0], mapq=grid[i, 1], name=b"t", at=i)
    return w.finish()


# ---- 2a, small: stream lengths around a chunk
def _plain_block(w, n, first_pos=1000, l=150, **kw):
    rng = np.random.default_rng(n + l)
    w.block(first_pos + 2 * np.arange(n), [("M", l)], rng.integers(2, 42, (n, l)), nibbles=rng.choice(np.array([1, 2, 4, 8], np.uint8), (n, l)),
            reverse=np.arange(n) % 2 == 1, name=b"r%07d" % 0, **kw)


LENGTH_CASES = ["n%32768=0 (last record ends on a chunk boundary)", "n%32768=1", "n%32768=3", "n%32768=4", "n%32768=32767",
                "first record starts on a chunk boundary", "header of three chunks and one record",
                "header only, under one chunk", "header only, one chunk", "header only, over one chunk"]


@functools.lru_cache(maxsize=None)
def length_bam(case):
    refs = (("chr1", 250_000_000),)
    text = b"@HD\tVN:1.6\n"
    base = bs.BamWriter.header_length(refs, len(text))
    if case.startswith("n%32768="):
        rem = int(case.split("=")[1].split(" ")[0])
        w = bs.BamWriter(refs, text)
        _plain_block(w, 300)
        gap = (rem - w.offset) % bs.CHUNK
        w.filler(gap if gap >= 48 else gap + bs.CHUNK, 2000)
        bam = w.finish()
        assert len(bam.array) % bs.CHUNK == rem and bam.n_chunks >= 3
    elif case == "first record starts on a chunk boundary":
        w = bs.BamWriter(refs, text + bs.co_line(bs.CHUNK - base))
        _plain_block(w, 300)
        bam = w.finish()
        assert bam.at[0] == bs.CHUNK
    elif case == "header of three chunks and one record":
        w = bs.BamWriter(refs, text + b"".join(bs.co_line(4000) for _ in range(17)))
        _plain_block(w, 1)
        bam = w.finish()
        assert bam.at[0] // bs.CHUNK == 2 and bam.n_chunks == 3
    else:
        pad = {"header only, under one chunk": 0, "header only, one chunk": bs.CHUNK - base, "header only, over one chunk": bs.CHUNK - base + 7232}[case]
        bam = bs.BamWriter(refs, text + (bs.co_line(pad) if pad else b"")).finish()
        assert bam.n_records == 0 and len(bam.array) == base + pad
    return bam


# ---- 2d
DEFECTS = {
    # name: (block() fields of the defective record, the code's message, l_ref of chr1)
    "position 0": (dict(pos=[0], cigar=[("M", 150)]), "Position must be greater than 0.", 1_000_000),
    "span one longer": (dict(pos=[1500], cigar=[("M", 151)]), "CIGAR does not match the read", 1_000_000),
    "span one shorter": (dict(pos=[1500], cigar=[("M", 100), ("I", 49)]), "CIGAR does not match the read", 1_000_000),
    # (the aligned bases end inside the last block the map can name, the skip behind them carries the read past 2^31 - 1: a read whose
    # ALIGNED bases pass it is refused as well, but as one past the block map, which the decode meets first)
    "past 2^31 - 1": (dict(pos=[2147482800], cigar=[("M", 150), ("N", 1000)]), "read runs past position 2^31 - 1", 2 ** 31 - 1),
    "past the block map": (dict(pos=[1_070_001 + 1000], cigar=[("M", 150)]), "far past the end of its reference sequence", 1_000_000),
}
N_REFUSAL = 600     # 270-byte records: five chunks


@functools.lru_cache(maxsize=None)
def refusal_bam(defects, skipped_twins=False, l_ref=None):
    """600 plain kept reads with the defective records of `defects` ((name, index) pairs) among them.  skipped_twins: the defective
    records are not kept (unmapped, or of the other reference sequence) -- two of each."""
    if l_ref is None:
        l_ref = max([DEFECTS[d][2] for d, _ in defects] + [1_000_000])
    w = bs.BamWriter((("chr1", l_ref), ("chr2", 1_000_000)))
    special = {}
    for d, i in defects:
        if skipped_twins:
            special[i] = (d, dict(flag=0x4))
            special[i + 1] = (d, dict(ref_id=1))
        else:
            special[i] = (d, {})
    plain = np.array([i for i in range(N_REFUSAL) if i not in special])
    _plain_block(w, len(plain), at=plain)
    for i, (d, kw) in special.items():
        w.block(quals=[30] * 150, seq="ACGTA" * 30, name=b"r%07d" % 1, at=[i], **dict(DEFECTS[d][0], **kw))
    bam = w.finish()
    assert bam.n_chunks >= 4
    return bam


# ---- 2e
def any_cigar_reads(seed):
    """random_reads of test_read_store.py; the reads it gave per-base directions get an XD string instead (runs over the expanded CIGAR)."""
    rng = np.random.default_rng(seed)
    reads = random_reads(rng, 1500, 20, 3800, exotic=False)
    for r in reads:
        if r.pop("dirs", None) is not None:
            total = sum(l for _, l in r["cigar"])
            cuts = sorted(set(int(x) for x in rng.integers(1, max(total, 2), int(rng.integers(0, 4)))) | {total})
            runs, last = [], 0
            for cpos in cuts:
                if cpos > last:
                    runs.append((cpos - last, "FRS"[int(rng.integers(0, 3))]))
                    last = cpos
            r["xd"] = bs.xd_of_runs(runs)
    return reads


def bam_of_reads(reads, l_ref=1_000_000):
    w = bs.BamWriter((("chr1", l_ref),))
    for i, r in enumerate(reads):
        w.read(r, name=b"q%06d" % i, aux=b"NMC\x02" if i % 2 else b"", aux_after=b"ASi" + struct.pack("<i", i) if i % 3 else b"")
    return w.finish()


# ---------------------------------------------------------------- CPU: the writer against the plain reader
def test_writer_of_record_shapes_agrees_with_the_plain_reader():
    bam = shapes_bam()
    assert 1500 < bam.n_records < 2600
    _writer_agrees_with_plain_reader(bam, [(0, 1, True, False), (1, 1, True, False)])
    want = bam.expected(0)["arrays"]
    seen = set()
    for s, e in zip(want["seq_offset"][:-1], want["seq_offset"][1:]):
        seen |= {(chr(b), k & 1) for k, b in enumerate(want["bases"][s:e].tolist())}
    assert {(c, p) for c in bs.SEQ_LETTERS for p in (0, 1)} <= seen                                   # every nibble at even and odd indexes
    assert set(np.diff(want["seq_offset"]).tolist()) >= set(SEQ_LENGTHS)
    ops = bam.expected(1)["arrays"]
    assert set(b"MIDNSHP=X?") == set(ops["cigar_op"].tolist()) and ops["cigar_len"].max() == 2 ** 28 - 1 and 0 in np.diff(ops["seq_offset"])
    assert {0, 41, 93, 254, 255} <= set(want["quals"].tolist())


def test_writer_of_the_filter_table_agrees_with_the_plain_reader():
    bam = filter_bam()
    _writer_agrees_with_plain_reader(bam, FILTER_SETTINGS + [(1, 1, True, False)])
    assert len({bam.expected(*s)["reads"] for s in FILTER_SETTINGS}) > 8


@pytest.mark.parametrize("case", LENGTH_CASES)
def test_writer_of_the_stream_length_cases_agrees_with_the_plain_reader(case):
    _writer_agrees_with_plain_reader(length_bam(case), [(0, 1, True, False)])


def test_writer_of_refusals_and_any_cigar_reads_agrees_with_the_plain_reader():
    for d in DEFECTS:
        _writer_agrees_with_plain_reader(refusal_bam(((d, 125),)), [(0, 1, True, False)])
        _writer_agrees_with_plain_reader(refusal_bam(((d, 125),), skipped_twins=True), [(0, 1, True, False)])
    reads = any_cigar_reads(41)
    assert sum("xd" in r for r in reads) > 200
    bam = bam_of_reads(reads)
    _writer_agrees_with_plain_reader(bam, [(0, 1, True, False)])
    batch = _abi.ReadBatch([dict(r) for r in reads])         # the host-fed form of the same reads: the same arrays, directions included
    want = bam.expected(0)
    _same_batch({k: getattr(batch, k) for k in ARRAYS}, want["arrays"])
    np.testing.assert_array_equal(batch.directions, want["directions"])
    np.testing.assert_array_equal(batch.deletion_directions, want["deletion_directions"])


LARGE = (257, 1024, 1025, 2049)


@functools.lru_cache(maxsize=2)
def large(n_chunks):
    bam = bs.large_case(n_chunks)
    return bam, bam.expected(0), bam.file(0)


def test_the_large_cases_are_what_the_chunk_count_tests_rely_on():
    """The chunk counts; runs of records of the other reference sequence that leave two whole chunks without a kept read and lie across
    the chunk boundaries 255|256 and 1023|1024 (the edges of the entry kernels' first workgroup and of the scans' first pass), with chunks
    256 and 1024 -- the last chunk of the 257 and of the 1025 case -- still holding reads, whose places are the first to depend on the
    second workgroup and on the carried sums; and counts that differ from chunk to chunk: a change
    to the writer cannot quietly turn these cases into easy ones.  (257 chunks also against the plain reader, record for record.)"""
    for n in LARGE:
        bam = bs.large_case(n)
        assert bam.n_chunks == n and bam.n_chunks == (len(bam.array) + 32767) // 32768
        kept = bam.kept_per_chunk(0)
        edges = bs.zero_kept_edges(n)
        assert edges == {257: [256], 1024: [256, 1023], 1025: [256, 1024], 2049: [256, 1024]}[n]
        zero = np.flatnonzero(kept == 0).tolist()
        assert zero == sorted(c - k for c in edges for k in (1, 2))          # two whole chunks in front of each edge, and no others
        for c in edges:                                                     # the run reaches across the edge; chunk c still has reads to place
            first_kept = bam.at[bam.keep(0) & (bam.at >= c * bs.CHUNK)].min()
            assert c * bs.CHUNK + bs.ZERO_KEPT_REACH <= first_kept < c * bs.CHUNK + bs.ZERO_KEPT_REACH + 4096 and kept[c] > 20
        exp = bam.expected(0)
        a = exp["arrays"]
        # per chunk: reads, CIGAR operations, bases, insertions longer than the inline record: all of them vary
        chunk_of_read = bam.at[exp["index"]] // bs.CHUNK
        for per_read in (np.ones(exp["reads"]), np.diff(a["cigar_offset"]), np.diff(a["seq_offset"]),
                         np.add.reduceat((a["cigar_op"] == ord("I")) * (a["cigar_len"] > 32) * a["cigar_len"].astype(np.int64), a["cigar_offset"][:-1])):
            per_chunk = np.bincount(chunk_of_read, weights=per_read, minlength=n)
            assert len(np.unique(per_chunk)) > 40
        assert set("MIDS=X") <= set(map(chr, a["cigar_op"].tolist())) and set(np.diff(a["seq_offset"]).tolist()) == {36, 150, 151, 250}
        assert set(np.diff(a["cigar_offset"]).tolist()) == {1, 2, 3, 4} and exp["skipped"] > 100
        assert (np.diff(a["position"]) >= 0).all() and bam.size.max() < 4096     # (sorted; records the guessed chain can take)
        if n == 257:
            _writer_agrees_with_plain_reader(bam, [(0, 1, True, False)])


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    return torch


def _decode_equals(c, data, want, ref_id=0, **filt):
    counts = c.bam_decode(data, ref_id, **filt)
    assert {k: counts[k] for k in ("reads", "skipped", "cigar_ops", "bases")} == {k: want[k] for k in ("reads", "skipped", "cigar_ops", "bases")}
    _same_batch(c.bam_fetch(), want["arrays"])
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("n_chunks", LARGE)
def test_chunk_counts_past_one_workgroup_and_one_scan_pass(gpu, n_chunks):
    """257 chunks: a second workgroup of bam_entry_guess_kernel / bam_entry_check_kernel.  1024 / 1025 / 2049: none, one and two carries
    of bam_scan3_kernel / bam_scan_ll_kernel, which place every chunk's reads, CIGAR operations and bases in the batch.  Counts and
    every fetched array (the closing offsets included) equal the writer's; the chain is the guessed one, and at 1025 chunks the hopped
    one gives the same."""
    bam, want, data = large(n_chunks)
    with engine.HipVariantCaller(_abi.default_config()) as c:
        assert _decode_equals(c, data, want)["chain"] == "guessed"
        if n_chunks == 1025:
            with env(PISCES_HIP_BAM_SERIAL_CHAIN=1):
                assert _decode_equals(c, data, want)["chain"] == "hopped"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "log"])
def test_decoded_add_at_1025_chunks_equals_the_host_fed_add(gpu, path):
    """What the decode derives for the add (slots, fslots, pool bytes, block-map bits) is placed by the scans' carried sums too:
    AddDecodedReads + CallWithAlleles (min_coverage 1, random reference, reference calls on) equals, byte for byte and in Stats(), a
    handle fed the writer's expected batch through AddAlleleCounts."""
    bam, want, data = large(1025)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(9).integers(0, 4, 22_000)]
    cfg = _abi.default_config(min_coverage=1, low_depth_filter=1, include_reference_calls=1)
    outs = []
    with env(PISCES_HIP_READ_PATH="log" if path == "log" else None):
        for how in ("decoded", "host"):
            with engine.HipVariantCaller(cfg) as c:
                c.SetReference(ref)
                if how == "decoded":
                    assert c.bam_decode(data, 0)["reads"] == want["reads"]
                    c.AddDecodedReads()
                else:
                    c.AddAlleleCounts(_abi.ReadBatch.from_arrays(**want["arrays"]))
                rows, alleles = c.CallWithAlleles(None, capacity=1 << 18)
                outs.append((rows, alleles, c.Stats()))
    (got, got_alleles, got_stats), (exp, exp_alleles, exp_stats) = outs
    assert len(exp) > 20_000 and any(len(a[1]) > 32 for a in exp_alleles) and any(len(a[0]) > 1 for a in exp_alleles)
    assert got.tobytes() == exp.tobytes() and got_alleles == exp_alleles
    assert got_stats["reads"] == want["reads"] and got_stats["TotalNumCalled"] == exp_stats["TotalNumCalled"] and \
        got_stats["TotalNumCollapsed"] == exp_stats["TotalNumCollapsed"]
    assert got_stats["reads_skipped"] == want["skipped"]


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["guessed", "hopped"])
@pytest.mark.parametrize("case", LENGTH_CASES)
def test_stream_lengths_around_a_chunk(gpu, case, chain):
    """Stream lengths of every remainder that matters to a 4-byte block_size at a chunk's end, records and headers that end or start on
    a boundary, a header of three chunks, and streams that are a header and nothing else (no reads, no error, an add that adds
    nothing), with the guessed and with the hopped chain."""
    bam = length_bam(case)
    want = bam.expected(0)
    with env(PISCES_HIP_BAM_SERIAL_CHAIN=1 if chain == "hopped" else None):
        with engine.HipVariantCaller(_abi.default_config()) as c:
            counts = _decode_equals(c, bam.file(1), want)
            if chain == "hopped":
                assert counts["chain"] == "hopped"
            if bam.n_records == 0:
                assert counts["reads"] == 0 and counts["skipped"] == 0
            c.AddDecodedReads()
            assert c.Stats()["reads"] == want["reads"]


@pytest.mark.gpu
def test_every_record_shape_is_decoded_and_added(gpu):
    """shapes_bam(): the decode's arrays and direction maps against the writer for both reference sequences; for the well-formed reads
    of chr1 the decoded add gives the counts of the host-fed add of the same arrays."""
    bam = shapes_bam()
    data = bam.file(1)
    cfg = _abi.default_config(expect_stitched_reads=1)
    hi = int(bam.pos.max()) + 400
    with engine.HipVariantCaller(cfg) as c:
        for ref_id in (1, 0):
            want = bam.expected(ref_id)
            _decode_equals(c, data, want, ref_id)
            if want["directions"] is None:
                assert c.bam_fetch_directions() is None
            else:
                dirs, dd = c.bam_fetch_directions()
                np.testing.assert_array_equal(dirs, want["directions"])
                np.testing.assert_array_equal(dd, want["deletion_directions"])
        c.AddDecodedReads()
        got = c.GetCounts(1, hi)
        assert c.Stats()["reads"] == want["reads"]
    with engine.HipVariantCaller(cfg) as c:
        c.AddAlleleCounts(_abi.ReadBatch.from_arrays(directions=want["directions"], deletion_directions=want["deletion_directions"], **want["arrays"]))
        exp = c.GetCounts(1, hi)
    assert exp.sum() > 100_000
    np.testing.assert_array_equal(got, exp)


@pytest.mark.gpu
def test_should_skip_read_truth_table(gpu):
    """Every row of filter_bam() under min_map_quality x skip_duplicates x only_proper_pairs for two reference sequences: the kept
    reads are the writer's, and kept + skipped are the records of that reference sequence (a record of ref_id -1 is nobody's)."""
    bam = filter_bam()
    data = bam.file(1)
    with engine.HipVariantCaller(_abi.default_config()) as c:
        for ref_id, mq, dups, proper in FILTER_SETTINGS:
            want = bam.expected(ref_id, mq, dups, proper)
            counts = _decode_equals(c, data, want, ref_id, min_map_quality=mq, skip_duplicates=dups, only_proper_pairs=proper)
            assert counts["reads"] + counts["skipped"] == int((bam.ref_id == ref_id).sum()) == 22 * 7 * 2


def _refused(c, add, needle, index=None, flush=True):
    before = c.Stats()
    with pytest.raises(engine.PiscesHipError) as e:
        add()
    assert e.value.code == _abi.E_INVALID_ARG and needle in e.value.message, e.value.message
    if index is not None:
        assert f"(read {index} of the decoded batch)" in e.value.message, e.value.message
    assert c.Stats() == before
    if flush:
        assert len(c.Call()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_one_defective_read_is_refused_at_the_add(gpu, defect):
    """A well-formed record with one semantic defect among 600 good ones: bam_decode succeeds, AddDecodedReads refuses the batch with
    that defect's message and the read's index, nothing is added, and a clean file through the same handle gives what a fresh handle
    gives.  The same records when they are skipped (unmapped, other reference sequence) are not reported.  The host-fed add of the
    fetched arrays refuses the first four with the same message on both read paths; the fifth is the decode's own limit (its block map
    ends 70 000 positions behind the reference sequence the header names): the host-fed add, which knows no such length, takes the
    read and counts it."""
    needle = DEFECTS[defect][1]
    bad, clean = refusal_bam(((defect, 125),)), refusal_bam((), l_ref=DEFECTS[defect][2])
    twins = refusal_bam(((defect, 125),), skipped_twins=True)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(4).integers(0, 4, 3000)]
    cfg = _abi.default_config(min_coverage=1, low_depth_filter=1)
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(ref)
        want = bad.expected(0)
        _decode_equals(c, bad.file(1), want)
        fetched = c.bam_fetch()
        _refused(c, c.AddDecodedReads, needle, 125)
        _decode_equals(c, twins.file(1), twins.expected(0))
        assert twins.expected(0)["reads"] == N_REFUSAL - 2 and twins.expected(0)["skipped"] == 1
        c.AddDecodedReads()
        assert c.Stats()["reads"] == N_REFUSAL - 2
        rows_twins = c.CallWithAlleles()
    with engine.HipVariantCaller(cfg) as c:                    # after a refusal, the same handle
        c.SetReference(ref)
        c.bam_decode(bad.file(1), 0)
        _refused(c, c.AddDecodedReads, needle, 125)
        c.bam_decode(clean.file(1), 0)
        c.AddDecodedReads()
        again = c.CallWithAlleles() + (c.Stats(),)
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(ref)
        c.bam_decode(clean.file(1), 0)
        c.AddDecodedReads()
        fresh = c.CallWithAlleles() + (c.Stats(),)
    assert len(fresh[0]) > 1000 and again[0].tobytes() == fresh[0].tobytes() and again[1:] == fresh[1:] and len(rows_twins[0]) > 1000
    for path in (None, "log"):
        with env(PISCES_HIP_READ_PATH=path):
            with engine.HipVariantCaller(cfg) as c:
                def add():
                    c.AddAlleleCounts(_abi.ReadBatch.from_arrays(**fetched))
                if defect != "past the block map":
                    _refused(c, add, needle, flush=False)
                else:
                    add()
                    assert c.Stats()["reads"] == N_REFUSAL and c.GetCounts(int(DEFECTS[defect][0]["pos"][0]), 150).sum() == 150


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [("position 0", "span one longer"), ("span one shorter", "position 0"), ("past the block map", "span one longer")])
def test_of_two_defective_reads_the_lower_index_is_named(gpu, first, second):
    """Two defective reads of different kinds in different chunks: first_error is an atomicMin of read * 8 + code over all chunks, the
    lower read index is named whichever workgroup reports last -- the lower read among the first records of chunk 1 and the higher among
    the last of chunk 4 (which its workgroup reaches some thirty records later), and the other way round; each with the two kinds in
    both orders."""
    at = refusal_bam(()).at
    early1, late1 = int(np.searchsorted(at, bs.CHUNK)) + 1, int(np.searchsorted(at, 2 * bs.CHUNK)) - 2
    early4, late4 = int(np.searchsorted(at, 4 * bs.CHUNK)) + 1, int(np.searchsorted(at, 5 * bs.CHUNK)) - 2
    for a, b in ((first, second), (second, first)):
        for lo, hi in ((early1, late4), (late1, early4)):
            bam = refusal_bam(((a, lo), (b, hi)))
            assert bam.at[lo] // bs.CHUNK == 1 and bam.at[hi] // bs.CHUNK == 4 and bam.at[lo + (3 if lo == late1 else -3)] // bs.CHUNK != 1
            with engine.HipVariantCaller(_abi.default_config()) as c:
                _decode_equals(c, bam.file(1), bam.expected(0))
                _refused(c, c.AddDecodedReads, DEFECTS[a][1], lo, flush=False)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["guessed", "hopped"])
@pytest.mark.parametrize("what", ["l_read_name 0", "block_size smaller than the record's fields", "a record longer than a chunk"])
def test_records_bam_decode_itself_refuses(gpu, what, chain):
    """A record without a name, one whose block_size does not hold its name, CIGAR and bases, and one longer than kBamMaxRecord are
    refused by pisces_hip_bam_decode with a message of its own, whichever way the chain is cut."""
    w = bs.BamWriter((("chr1", 1_000_000),))
    _plain_block(w, 300)
    if what == "l_read_name 0":
        w.block([1700], [("M", 150)], [30] * 150, seq="ACGTA" * 30, raw_name=b"")
    elif what == "a record longer than a chunk":
        w.block([1700], [("M", 22000)], [30] * 22000, seq="ACGTA" * 4400)
    _plain_block(w, 300, first_pos=1800)
    bam = w.finish()
    stream = bam.array.copy()
    if what == "block_size smaller than the record's fields":
        stream[bam.at[400] + 20:bam.at[400] + 24] = np.frombuffer(struct.pack("<i", 150 + 100_000), np.uint8)   # l_seq says more than block_size holds
    assert bam.n_chunks >= 4
    with env(PISCES_HIP_BAM_SERIAL_CHAIN=1 if chain == "hopped" else None):
        with engine.HipVariantCaller(_abi.default_config()) as c:
            with pytest.raises(engine.PiscesHipError) as e:
                c.bam_decode(bs.bgzf(stream), 0)
            assert e.value.code == _abi.E_INVALID_ARG and "bam_decode" in e.value.message
            with pytest.raises(engine.PiscesHipError):
                c.AddDecodedReads()                              # (no decoded batch)


@pytest.mark.gpu
@pytest.mark.parametrize("min_bq", [20, 30])
@pytest.mark.parametrize("call_mnvs", [0, 1], ids=["snv_indel", "mnv"])
def test_any_cigar_from_bam_bytes_equals_the_host_fed_add(gpu, call_mnvs, min_bq):
    """The seeded any-CIGAR reads of test_read_store.py written as BAM (some stitched: XD tags), decoded, added and called over four
    1000-locus blocks in two flushes: records, allele strings and Stats() equal the host-fed add of the same reads, on the read store
    and on the log chain, and the counts are the oracle's."""
    reads = any_cigar_reads(41 + call_mnvs)
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(6).integers(0, 4, 4400)]
    cfg = _abi.default_config(call_mnvs=call_mnvs, min_base_call_quality=min_bq, min_coverage=1, low_depth_filter=1, expect_stitched_reads=1)
    parts = [reads[:800], reads[800:]]
    files = [bam_of_reads(p).file(1) for p in parts]
    ups = [reads[799]["pos"] - 1, None]
    batches = [_abi.ReadBatch(p) for p in parts]                # (this also leaves every xd read its per-base dirs, for the oracle)
    exp_counts = oracle_counts(reads, 1, 4200, min_bq=min_bq)
    outs = {}
    for path in (None, "log"):
        for how in ("decoded", "host"):
            with env(PISCES_HIP_READ_PATH=path):
                with engine.HipVariantCaller(cfg) as c:
                    c.SetReference(ref)
                    recs, alleles = [], []
                    for k in range(2):
                        if how == "decoded":
                            assert c.bam_decode(files[k], 0)["reads"] == len(parts[k])
                            c.AddDecodedReads()
                        else:
                            c.AddAlleleCounts(batches[k])
                        r, a = c.CallWithAlleles(ups[k], capacity=1 << 15)
                        recs.append(r)
                        alleles += a
                    outs[path, how] = (np.concatenate(recs), alleles, c.Stats())
    want = outs[None, "host"]
    assert len(want[0]) > 3000 and want[2]["reads"] == len(reads)
    for key, got in outs.items():
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2], key
    with engine.HipVariantCaller(cfg) as c:                    # the counts, nothing flushed
        for data in files:
            c.bam_decode(data, 0)
            c.AddDecodedReads()
        np.testing.assert_array_equal(c.GetCounts(1, 4200).reshape(exp_counts.shape), exp_counts)
