"""The hand-off of pisces_hip_add_device_reads (one launch, add_fused_kernel; surface_store.inc.h), at the three places where the host and
the launch meet without the stream between them:

A. the verdict.  The host polls one word in pinned memory and then reads the keys of the touched blocks beside it: the keys of EVERY wave of
   the collecting workgroup have to be there before the word is.  32 consecutive adds whose sets of touched blocks differ, so that a key left
   over from the launch before is a block that is never registered (its reads missing from the flush) and one that should not exist.
B. the copy contract (include/pisces_hip.h: the arrays "are copied: the caller may reuse them when the call returns").  The verdict comes
   from the launch's read role; its stream and misc roles may still be reading the caller's arrays.  The caller's arrays are overwritten
   the moment the call returns; the counts must be those of what was handed over.
C. a position grid that was kept back (deferred_grid) and whose segment is retired by a flush that launched nothing over the store.

The race window of B was measured once on the parent of the commit that added the wait (PISCES_ADD_STAMPS build, MI355X): the figures are
in test_the_callers_arrays_may_be_overwritten_when_the_add_returns and in DESIGN.md section 3.10."""
import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc
from tests.test_read_store import STORE_MODES, env, random_reads

pytestmark = pytest.mark.gpu

OTHER = np.zeros(256, np.uint8)   # a different base of A C G T for every base
for _a, _b in zip(b"ACGT", b"CGTA"):
    OTHER[_a] = _b


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


# ---- A. touched blocks survive a changing key set -------------------------------------------------------------------------------------
ROUNDS, BLOCKS, BLOCK_SIZE, READ_LEN = 32, 20_000, 1000, 12


@pytest.fixture(scope="module")
def key_rounds():
    """32 batches of about 6 000 twelve-base 12M reads, each read in a block of its own, the blocks a fresh seeded subset of 20 000 every
    round: fewer keys than the 8 192 the launch lists in pinned memory (the keys_out path), enough of them that all four waves of the
    collecting workgroup write some, and a different set — and a different number — after every launch.  Every third read carries one
    mismatch, so that rows are made."""
    rng = np.random.default_rng(20260)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, BLOCKS * BLOCK_SIZE + 64)]
    batches = []
    for _ in range(ROUNDS):
        n = int(rng.integers(5600, 6400))
        keys = np.sort(rng.choice(BLOCKS, n, replace=False)) + 1
        pos = (keys - 1) * BLOCK_SIZE + rng.integers(1, BLOCK_SIZE - READ_LEN, n)
        bases = ref[(pos - 1)[:, None] + np.arange(READ_LEN)[None, :]].copy()
        hit = np.arange(0, n, 3)
        at = rng.integers(0, READ_LEN, len(hit))
        bases[hit, at] = OTHER[bases[hit, at]]
        batches.append(_abi.ReadBatch.from_arrays(
            pos.astype(np.int32), rng.integers(0, 2, n).astype(np.uint8), np.arange(n + 1, dtype=np.int32), np.full(n, ord("M"), np.uint8),
            np.full(n, READ_LEN, np.uint32), np.arange(n + 1, dtype=np.int32) * READ_LEN, bases.reshape(-1), np.full(n * READ_LEN, 37, np.uint8)))
    return ref, batches, {}


def _rounds_run(ref, batches, how, environ):
    from pisces_amd import engine
    out = []
    with env(PISCES_HIP_READ_PATH=None, **environ):
        with engine.HipVariantCaller(_abi.default_config(min_coverage=1, low_depth_filter=1, include_reference_calls=0)) as c:
            c.SetReference(ref)
            for batch in batches:
                (c.AddDeviceReads if how == "device" else c.AddAlleleCounts)(batch)
                rows, alleles = c.CallWithAlleles(None, capacity=1 << 14)
                out.append((rows.tobytes(), alleles, c.Stats()))
    return out


@pytest.mark.parametrize("how,mode", [("device", mode) for mode in STORE_MODES] + [("host checked on the device", "default")])
def test_touched_blocks_of_consecutive_adds_with_changing_key_sets(torch_cuda, key_rounds, how, mode):
    """32 x (AddDeviceReads, CallWithAlleles(None)) on one handle == the same rounds through pisces_hip_add_reads with the host's pass over
    the CIGARs (PISCES_HIP_DEVICE_CHECKS=0): records, allele strings and Stats() are the same bytes after every round and at the end.  A key
    of the launch before read in place of this launch's (the word the host polls overtaking the keys of waves 1-3) registers a block without
    reads and leaves one with reads unregistered: rows missing from this round's flush and TotalNumCalled off.  On the parent of the fix this
    is statistical, not certain; the ordering itself is shown by the kernel's assembly (profiles/add_fused_handoff_isa.txt)."""
    ref, batches, cache = key_rounds
    if mode not in cache:
        cache[mode] = _rounds_run(ref, batches, "host", dict(PISCES_HIP_DEVICE_CHECKS=0, **STORE_MODES[mode]))
    want = cache[mode]
    assert all(len(w[0]) // _abi.CALLED_ALLELE_DTYPE.itemsize > 1500 for w in want)
    assert want[-1][2]["reads"] == sum(b.n_reads for b in batches)
    got = _rounds_run(ref, batches, "device" if how == "device" else "host",
                      dict(STORE_MODES[mode], **({} if how == "device" else {"PISCES_HIP_DEVICE_CHECKS": 1})))
    for r, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (r, g[2], w[2])
        assert g[1] == w[1] and g[0] == w[0], r


# ---- B. the caller may reuse its arrays when the call returns -------------------------------------------------------------------------
LONG_READS, LONG_LEN, LONG_REVERSE = 8192, 62_500, 3072


@pytest.fixture(scope="module")
def long_batch(torch_cuda):
    """A batch whose read role is short and whose stream role is long: 8 192 reads of 62 500 bases, all 62500M at position 1, bases equal
    to the reference, quality 35, the first 3 072 reverse — 32 read workgroups against 1 GB to read and 1.5 GB to write.  (The read role
    walks a read's qualities in one lane: 256 reads of 1 000 000 bases keep its collector busy until 12-28 us before the stream role
    ends, and 4 096 reads of 62 500 leave 75-95 us; this shape leaves 284-294 us.)  With it, on the
    device, what the caller's arrays are overwritten with: every base another one of A C G T, quality 2, the reverse bit flipped (all of
    them valid values; positions, offsets and CIGARs are never touched — the flush walks those unchecked)."""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, LONG_LEN)]
    n, ln = LONG_READS, LONG_LEN
    flags = (np.arange(n) < LONG_REVERSE).astype(np.uint8)
    small = dict(position=np.ones(n, np.int32), flags=flags, cigar_offset=np.arange(n + 1, dtype=np.int32), cigar_op=np.full(n, ord("M"), np.uint8),
                 cigar_len=np.full(n, ln, np.uint32), seq_offset=np.arange(n + 1, dtype=np.int32) * ln)
    dev = "cuda:0"
    ref_d = torch.from_numpy(ref.copy()).to(dev)
    other = torch.from_numpy(OTHER).to(dev)
    bases2 = other[ref_d.long()].repeat(n)
    quals2 = torch.full((n * ln,), 2, dtype=torch.uint8, device=dev)
    flags2 = torch.from_numpy(flags ^ 1).to(dev)
    windows = [1, ln - 63] + sorted(int(x) for x in np.random.default_rng(78).integers(65, ln - 128, 6))
    torch.cuda.synchronize()
    return dict(ref=ref, ref_d=ref_d, small=small, bases2=bases2, quals2=quals2, flags2=flags2, windows=windows)


def _check_counts_are_the_batch_as_handed_over(c, ref, windows, n_reads, n_reverse, quality=35):
    """Closed form, without the oracle: every position is covered by every read with the reference's base, in the direction the read had.
    The base-quality sums are sums of Math.Pow(10, -(int)q / 10f) (RegionState._sumOfAlleleBaseQualities), kept in fixed point and exact to
    8 ulp a cell (test_base_quality_sums_are_exact_and_the_same_from_run_to_run); the eleven anchor cells added up here add as many roundings:
    rtol 1e-12 is hundreds of times that, and a base counted at the overwritten quality 2 is off by a factor of 2 000."""
    term = float(np.float64(10.0) ** np.float64(np.float32(-quality) / np.float32(10.0)))
    for lo in windows:
        counts = c.GetCounts(lo, 64).sum(axis=3)              # [64][AlleleType][DirectionType]
        sums = c.GetBaseQualitySums(lo, 64).sum(axis=3)
        want = np.zeros((64, 6, 3), np.int64)
        for k in range(64):
            a = _abi.ALLELE_OF_BASE[chr(ref[lo - 1 + k])]
            want[k, a, _abi.DIR_FORWARD] = n_reads - n_reverse
            want[k, a, _abi.DIR_REVERSE] = n_reverse
        np.testing.assert_array_equal(counts, want, err_msg=f"window at {lo}")
        np.testing.assert_allclose(sums, want * term, rtol=1e-12, atol=0, err_msg=f"window at {lo}")
        assert int(counts.sum()) == 64 * n_reads


def _device_long_batch(torch, L, n=LONG_READS):
    from pisces_amd import engine
    up = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to("cuda:0")
    s = L["small"]
    return engine.DeviceReadBatch(up(s["position"]), up(s["flags"]), up(s["cigar_offset"]), up(s["cigar_op"]), up(s["cigar_len"], np.int32), up(s["seq_offset"]),
                                  L["ref_d"].repeat(n), torch.full((n * LONG_LEN,), 35, dtype=torch.uint8, device="cuda:0"))


def test_the_callers_arrays_may_be_overwritten_when_the_add_returns(torch_cuda, long_batch):
    """pisces_hip_add_device_reads returns; at once the caller's bases, qualities and flags are overwritten from a torch side stream (not
    the handle's).  The store must hold what was handed over: coverage 8 192 of the reference's base at every position, 5 120 forward and
    3 072 reverse, base-quality sums of 8 192 bases of quality 35, at eight 64-locus windows (the first and the last tile among them), and not one variant row.  An
    add that returns with the verdict while the launch's stream role is still reading (the parent of the fix) stores the other bases at
    quality 2 from wherever the overwrite overtakes the copy.

    The window, measured once (parent commit, PISCES_ADD_STAMPS build, MI355X, this batch, three adds; us from the launch's first start):
    "collector done" 158.1 / 142.0 / 141.3, the stream role's "last end" 451.9 / 428.9 / 425.5 — the parent's add returned 284-294 us before
    the caller's arrays had been read, twelve times the 20-25 us a host turn takes."""
    torch = torch_cuda
    from pisces_amd import engine
    L = long_batch
    b = _device_long_batch(torch, L)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with engine.HipVariantCaller(_abi.default_config(include_reference_calls=0)) as c:
        c.SetReference(L["ref"])
        c.AddDeviceReads(b)
        with torch.cuda.stream(side):
            b.tensors["bases"].copy_(L["bases2"], non_blocking=True)
            b.tensors["quals"].copy_(L["quals2"], non_blocking=True)
            b.tensors["flags"].copy_(L["flags2"], non_blocking=True)
        torch.cuda.synchronize()
        assert c.Stats()["reads"] == LONG_READS
        _check_counts_are_the_batch_as_handed_over(c, L["ref"], L["windows"], LONG_READS, LONG_REVERSE)
        rows, _ = c.CallWithAlleles(None, capacity=1 << 12)
        assert len(rows) == 0


def test_the_temporaries_of_a_host_batch_may_go_back_to_the_allocator_when_the_add_returns(torch_cuda, long_batch):
    """engine.AddDeviceReads of an _abi.ReadBatch uploads the arrays into temporary tensors, which go back to torch's caching allocator when
    the call returns.  Two tensors of the size of the bases are allocated right behind it and filled on torch's current stream — the
    allocator hands out the blocks it was just given back (large blocks: never one of the small arrays') — with the other bases, which are
    valid as bases and, 65 and more, as qualities.  Same closed form as above."""
    torch = torch_cuda
    from pisces_amd import engine
    L = long_batch
    s = L["small"]
    batch = _abi.ReadBatch.from_arrays(s["position"], s["flags"], s["cigar_offset"], s["cigar_op"], s["cigar_len"], s["seq_offset"],
                                       np.tile(L["ref"], LONG_READS), np.full(LONG_READS * LONG_LEN, 35, np.uint8))
    torch.cuda.synchronize()
    with engine.HipVariantCaller(_abi.default_config(include_reference_calls=0)) as c:
        c.SetReference(L["ref"])
        c.AddDeviceReads(batch)
        refill = [torch.empty_like(L["bases2"]).copy_(L["bases2"]) for _ in range(2)]
        torch.cuda.synchronize()
        assert all(int(t[-1]) == int(L["bases2"][-1]) for t in refill)
        _check_counts_are_the_batch_as_handed_over(c, L["ref"], L["windows"], LONG_READS, LONG_REVERSE)
        rows, _ = c.CallWithAlleles(None, capacity=1 << 12)
        assert len(rows) == 0


def test_the_arrays_and_ids_of_a_tracking_add_may_be_overwritten_when_it_returns(torch_cuda, long_batch):
    """pisces_hip_add_device_reads_amplicons on a tracking handle, the same batch with an amplicon id a read (0, 1, 2 in turn): bases,
    qualities, flags and the id tensor (ids 3, 4, 5) are overwritten when the call returns.  Counts as handed over, by direction and by
    amplicon."""
    torch = torch_cuda
    from pisces_amd import engine
    L = long_batch
    b = _device_long_batch(torch, L)
    ids = (np.arange(LONG_READS) % 3).astype(np.int32)
    ids_d, ids2 = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(ids + 3).to("cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with engine.HipVariantCaller(_abi.default_config(include_reference_calls=0)) as c:
        c.SetReference(L["ref"])
        c.SetAmpliconBiasFilter(0.01)
        c.AddDeviceReads(b, amplicon_ids=ids_d)
        with torch.cuda.stream(side):
            b.tensors["bases"].copy_(L["bases2"], non_blocking=True)
            b.tensors["quals"].copy_(L["quals2"], non_blocking=True)
            b.tensors["flags"].copy_(L["flags2"], non_blocking=True)
            ids_d.copy_(ids2, non_blocking=True)
        torch.cuda.synchronize()
        _check_counts_are_the_batch_as_handed_over(c, L["ref"], L["windows"], LONG_READS, LONG_REVERSE)
        per_id = [int((ids == k).sum()) for k in range(3)]
        for lo in L["windows"]:
            got_ids, cov, _ = c.GetCoverageByAmplicon(lo, 64)
            assert (got_ids == np.array([0, 1, 2, -1, -1, -1])).all() and (cov == np.array(per_id + [0, 0, 0])).all(), lo
        assert len(c.Call(None, capacity=1 << 12)) == 0


# ---- C. a segment retired without a reader takes its deferred grid with it ------------------------------------------------------------
INTERVAL = (100_001, 101_000)


@pytest.fixture(scope="module")
def retire_case():
    """Batch A: 3 000 reads x 50M in positions 1-900, outside the interval set, large enough for a segment of its own (store_place_batch:
    2 x 150 000 + 5 x 3 000 bytes >= 256 KiB) and without a candidate (one aligned run each: the flush has nothing to count for the spanning
    alleles either).  Batch B: 6 000 reads with arbitrary CIGARs inside the interval, about three times A's bytes: the pooled segment's blob
    is reallocated.  Expected rows of B alone from the oracle."""
    rng = np.random.default_rng(4242)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, INTERVAL[1] + 400)]
    na = 3000
    pos_a = np.sort(rng.integers(1, 901, na)).astype(np.int32)
    bases_a = ref[(pos_a - 1)[:, None] + np.arange(50)[None, :]].copy()
    a = _abi.ReadBatch.from_arrays(pos_a, rng.integers(0, 2, na).astype(np.uint8), np.arange(na + 1, dtype=np.int32), np.full(na, ord("M"), np.uint8),
                                   np.full(na, 50, np.uint32), np.arange(na + 1, dtype=np.int32) * 50, bases_a.reshape(-1), np.full(na * 50, 35, np.uint8))
    reads = random_reads(rng, 6000, INTERVAL[0], INTERVAL[1] - 200, with_dirs=False)
    for r in reads[::3]:   # reads that look like their reference (with a few mismatches), so that calls are made
        ln = len(r["seq"])
        if r["cigar"] == [("M", ln)]:
            seq = bytearray(ref[r["pos"] - 1:r["pos"] - 1 + ln].tobytes())
            for k in range(ln):
                if rng.random() < 0.02:
                    seq[k] = int(rng.choice(list(b"ACGT")))
            r["seq"] = bytes(seq)
    b = _abi.ReadBatch(reads)
    assert 2 * a.n_bases + 5 * len(a.cigar_op) >= 256 << 10 and b.n_bases > 2 * a.n_bases
    cfg = _abi.default_config(min_coverage=1, low_depth_filter=1)
    exp = orc.run_reads_schedule(b, ref, INTERVAL[0], INTERVAL[1] - INTERVAL[0] + 1, cfg, [], intervals=[INTERVAL])
    return ref, a, b, cfg, exp


def _retire_run(case, how, a_adds, environ):
    from pisces_amd import engine
    ref, a, b, cfg, _ = case
    with env(PISCES_HIP_READ_PATH=None, **environ):
        with engine.HipVariantCaller(cfg) as c:
            c.SetReference(ref)
            c.SetIntervals([INTERVAL])
            add = c.AddDeviceReads if how == "device" else c.AddAlleleCounts
            c.set_timing(True)
            for _ in range(a_adds):   # (every one a segment of its own; ONE flush retires them all)
                add(a)
            assert c.Stats()["reads"] == a_adds * a.n_reads
            assert len(c.Call(None)) == 0
            # (the flush's kernel over the store is the only timed launch of this surface: none was made, so nothing took store_view's way)
            skipped = c.kernel_time()[1] == 0
            add(b)
            rows, alleles = c.CallWithAlleles(None, capacity=1 << 15)
            launched = c.kernel_time()[1]
            stats = c.Stats()
    return rows, alleles, stats, skipped, launched


@pytest.mark.parametrize("a_adds", [1, 5], ids=["one segment retired: pooled", "five segments retired by one flush: four pooled, the fifth destroyed"])
def test_a_segment_retired_by_a_flush_that_launched_nothing_takes_its_grid_along(torch_cuda, retire_case, a_adds):
    """SetIntervals([(100 001, 101 000)]); device batch A in positions 1-900 becomes a segment of its own, its position grid is kept back
    (deferred_grid); Call(None) clips every tile of A's block away (call_blocks_enqueue returns at tiles.empty()): no kernel over the store,
    no store_view, and the segment is retired.  Device batch B takes the pooled segment and grows its blob.  The grid that was kept back
    has to run before its segment's buffers go (store_retire / store_commit_flush): rows, allele strings and Stats() equal the same sequence
    through host adds with the host's CIGAR pass, with and without PISCES_HIP_DEFER_GRID=0, and the rows are the oracle's for B alone.
    Five adds of A before the one flush: five segments of their own (the store holds up to seven closed ones), all dead at the flush;
    store_commit_flush retires them in order, the pool takes four and the fifth — the last one added, the one whose grid is still kept
    back: every add runs the grids of the adds before it — is destroyed, its buffers freed outright.  (On a library without the fix
    this launches read_shape_kernel through stale pointers: not to be run there.)"""
    want = _retire_run(retire_case, "host", a_adds, dict(PISCES_HIP_DEVICE_CHECKS=0))
    exp, exp_alleles, _ = retire_case[4]
    assert len(want[0]) > 500 and len(want[0]) == len(exp) and want[1] == exp_alleles
    for f in ("position", "total_coverage", "allele_support", "reference_support", "num_no_calls", "coverage_by_dir", "support_by_dir", "filter_bits",
              "info", "variant_qscore", "genotype_qscore"):
        assert (want[0][f] == exp[f]).all(), f
    assert (want[0]["position"] >= INTERVAL[0]).all() and (want[0]["position"] <= INTERVAL[1]).all()
    for environ in ({}, {"PISCES_HIP_DEFER_GRID": 0}):
        got = _retire_run(retire_case, "device", a_adds, environ)
        assert got[3], "the A-flush launched a kernel over the store: the path under test is no longer exercised"
        assert got[4] >= 1, "the B-flush shows no timed launch: the counter the line above relies on is dead"
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] and got[2] == want[2], environ
