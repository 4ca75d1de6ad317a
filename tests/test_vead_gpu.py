"""Scylla's read pass on the GPU (pisces_hip_vead_groups_device): device output == host entry (pisces_hip_vead_groups) == the plain-Python
statement (tests/vead_ref.py), compared as whole arrays: groups, state bytes, per-neighbourhood info.  tests/test_vead_cpu.py pins the host
entry and the statement to the reference's own facts.  The shapes are those at which the kernels can go wrong; each says why it is here."""
import os
import random
import types

import numpy as np
import pytest

from pisces_amd import _abi
from pisces_amd._native import PiscesHipError
from tests import vead_cases as V

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
G = V.golden()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def caller(torch_cuda):
    from pisces_amd import engine
    with engine.HipVariantCaller(_abi.default_config()) as c:
        yield c


def device_batch(reads_or_arrays):
    from pisces_amd import engine
    arrays = reads_or_arrays if hasattr(reads_or_arrays, "keys") else V.batch_of(reads_or_arrays)
    ns = types.SimpleNamespace(**{k: np.ascontiguousarray(arrays[k]) for k in ("position", "flags", "cigar_offset", "cigar_op", "cigar_len", "seq_offset", "bases", "quals")},
                               directions=None)
    b = engine.DeviceReadBatch.from_host(ns)
    if len(ns.position) == 0:
        b.n_reads = b.c.n_reads = 0   # (from_host pads empty arrays with one element to have a pointer)
    b.synchronize()
    return b


def run_device(torch, c, batch, rows, nbhd, caps, options=None):
    """one call into sentinel-filled device buffers: (n_out, raw buffers)"""
    from pisces_amd import engine
    dev = torch.device("cuda", c.device)
    with torch.cuda.stream(c.torch_stream()):
        full = lambda nbytes: torch.full((max(nbytes, 1) + 16,), SENTINEL, dtype=torch.uint8, device=dev)
        groups, states, info, n_out = full(caps[0] * 24), full(caps[1]), full(len(nbhd) * 32), full(24)
    out = engine.vead_out(groups, states, info, n_out, caps[0], caps[1])
    c.vead_groups_device(engine.vead_sites(rows), nbhd, out, batch=batch, options=options)
    c.synchronize()
    raw = {"groups": groups.cpu().numpy(), "states": states.cpu().numpy(), "info": info.cpu().numpy(), "n_out": n_out.cpu().numpy()[:24].view(np.int64).copy()}
    return raw


def device_groups(torch, c, batch, rows, nbhd, options=None, caps=(0, 0)):
    """the protocol a host follows: counts first (short capacities write only n_out and info), then the sizes they ask for; nothing is
    written past them"""
    raw = run_device(torch, c, batch, rows, nbhd, caps, options)
    ng, ns, err = (int(v) for v in raw["n_out"])
    assert err == 0 and ng >= 0
    if ng > caps[0] or ns > caps[1]:
        assert (raw["groups"] == SENTINEL).all() and (raw["states"] == SENTINEL).all(), "short capacities: only the counts come back"
        first = raw
        raw = run_device(torch, c, batch, rows, nbhd, (ng, ns), options)
        assert tuple(int(v) for v in raw["n_out"]) == (ng, ns, 0)
        assert raw["info"].tobytes() == first["info"].tobytes()
    assert (raw["groups"][ng * 24:] == SENTINEL).all() and (raw["states"][ns:] == SENTINEL).all() and (raw["info"][len(nbhd) * 32:] == SENTINEL).all()
    return {"groups": raw["groups"][:ng * 24].view(_abi.VEAD_GROUP_DTYPE).copy(), "states": raw["states"][:ns].copy(),
            "info": raw["info"][:len(nbhd) * 32].view(_abi.VEAD_INFO_DTYPE).copy(), "n_out": (ng, ns, err)}


def three_way(torch, c, reads, rows, nbhd, min_q=20, min_sites=1, batch=None):
    from pisces_amd import engine
    opts = engine.vead_options(min_base_call_quality=min_q, min_number_variants_in_read=min_sites)
    want = V.statement(reads, rows, nbhd, min_q, min_sites)
    host = engine.vead_groups(V.batch_of(reads), rows, nbhd, opts)
    V.assert_same(host, want, "host entry")
    got = device_groups(torch, c, batch if batch is not None else device_batch(reads), rows, nbhd, opts)
    V.assert_same(got, want, "device")
    return got


def test_every_golden_case_through_the_device(torch_cuda, caller):
    """the reference's own facts (tests/golden/vead_cases.json), each as a batch of its reads and one neighbourhood of its sites"""
    for case in G["finder_cases"]:
        if case["sites"]:
            three_way(torch_cuda, caller, [V.golden_read(case)], [tuple(s) for s in case["sites"]], [(0, len(case["sites"]))], case["min_q"])
    for case in G["check_cases"]:
        p, alt = case["segment"]
        three_way(torch_cuda, caller, [(p, [("M", len(alt))], alt, [30] * len(alt))], [tuple(case["look"])], [(0, 1)], 20, 0)
    for case in G["get_veads"]:
        reads = [(p, [("M", len(b))], b, [q] * len(b)) for p, b, q in case["reads"] if q >= case["min_map_quality"]]
        got = three_way(torch_cuda, caller, reads, [tuple(s) for s in case["sites"]], [(0, len(case["sites"]))], case["min_q"])
        assert [reads[r][0] for r in got["groups"]["first_read"]] == case["group_read_positions"]
    for case in G["group_veads"]:
        reads = [(100, [("M", len(b))], b, [30] * len(b)) for b in case["reads"]]
        got = three_way(torch_cuda, caller, reads, [tuple(s) for s in case["sites"]], [(0, len(case["sites"]))])
        assert list(got["groups"]["n_veads"]) == case["memberships"]
    for case in G["filters"]["clipped"]:
        reads = sorted((position, V.parse_cigar(cigar), "ACGT", [30] * 4) for position, cigar, _ in case["reads"])
        got = three_way(torch_cuda, caller, reads, [tuple(s) for s in case["sites"]], [(0, len(case["sites"]))])
        assert int(got["info"]["n_clipped_reads"][0]) == sum(1 for _, _, clipped in case["reads"] if clipped)


def overlapping_reads(rng, n, at=5000):
    """n reads that all cover [at, at + 40): every one of them lies in the range of a neighbourhood there"""
    reads = []
    for _ in range(n):
        lead = rng.randint(0, 3)
        cigar = ([("S", lead)] if lead and rng.random() < 0.3 else []) + [("M", 60)]
        n_bases = sum(k for _, k in cigar)
        reads.append((at - 10, cigar, "".join(rng.choice("ACGT") for _ in range(n_bases)), [rng.choice((19, 30, 30, 30)) for _ in range(n_bases)]))
    return reads


@pytest.mark.parametrize("n_reads", [0, 1, 63, 64, 65, 129])
def test_reads_in_range(torch_cuda, caller, n_reads):
    """0: no wave at all; 1: one lane; 63 / 64 / 65: a wave one short, full, and a second wave of one lane (the read the scan stops at adds
    one clip-tested pair, so 63 reads + that read fill a wave exactly); 129: three waves.  Reads before and behind the range stay outside."""
    rng = random.Random(n_reads)
    before = [(100 + i, [("M", 20)], "A" * 20, [30] * 20) for i in range(3)]
    behind = [(9000 + i, [("S", 2), ("M", 20)], "C" * 22, [30] * 22) for i in range(3)]
    reads = before + overlapping_reads(rng, n_reads) + behind
    rows = [(5000, "A", "C"), (5003, "AC", "A"), (5010, "G", "GTT"), (5020, "T", "T")]
    got = three_way(torch_cuda, caller, reads, rows, [(0, 4)])
    assert int(got["info"]["n_reads_used"][0]) == n_reads


@pytest.mark.parametrize("n_sites", [1, 31, 32, 33, 64, 65, 256])
def test_sites_at_the_word_edges_of_the_key(torch_cuda, caller, n_sites):
    """2 bits a site, 32 sites a 64-bit word: the last site of a word, the first of the next, two full words, and PISCES_VEAD_MAX_SITES.
    The reads differ only at single sites, the LAST one among them: a key that lost its tail would merge groups."""
    rng = random.Random(n_sites)
    base = "".join(rng.choice("ACGT") for _ in range(300))
    rows = [(2000 + i, "N" if base[i] == "N" else {"A": "C", "C": "G", "G": "T", "T": "A"}[base[i]], base[i]) for i in range(n_sites)]
    reads = []
    for k in range(40):
        b = list(base)
        for i in {n_sites - 1, (n_sites - 1) // 2, 0}:
            if (k >> (i % 3)) & 1:
                b[i] = rows[i][1]        # the reference base at that site
        if k % 7 == 3:
            b[n_sites - 1] = "G" if rows[n_sites - 1][1] != "G" and rows[n_sites - 1][2] != "G" else "T"
        reads.append((2000, [("M", 300)], "".join(b), [30] * 300))
    got = three_way(torch_cuda, caller, reads, rows, [(0, n_sites)])
    assert len(got["groups"]) >= 2 and len(got["states"]) == n_sites * len(got["groups"])


def test_more_than_max_sites_is_refused(torch_cuda, caller):
    from pisces_amd import engine
    rows = [(2000 + i, "A", "C") for i in range(_abi.VEAD_MAX_SITES + 1)]
    with pytest.raises(PiscesHipError) as e:
        run_device(torch_cuda, caller, device_batch([(2000, [("M", 10)], "A" * 10, [30] * 10)]), rows, [(0, len(rows))], (4, 1024))
    assert e.value.code == _abi.E_UNSUPPORTED and "PISCES_VEAD_MAX_SITES" in e.value.message
    with pytest.raises(PiscesHipError) as e:
        run_device(torch_cuda, caller, device_batch([(2000, [("M", 10)], "A" * 10, [30] * 10)]), rows[:2], [(1, 1)], (4, 1024))
    assert e.value.code == _abi.E_INVALID_ARG and "is empty" in e.value.message
    sites, alleles = engine.vead_sites(rows[:2])
    sites["ref_len"][0] = 0
    with pytest.raises(PiscesHipError) as e:
        run_device(torch_cuda, caller, device_batch([(2000, [("M", 10)], "A" * 10, [30] * 10)]), (sites, alleles), [(0, 2)], (4, 1024))
    assert e.value.code == _abi.E_INVALID_ARG and "below 1" in e.value.message


def test_neighbourhoods_that_share_reads_miss_all_reads_and_end_the_batch(torch_cuda, caller):
    """two neighbourhoods over the same reads (pairs, tables and keys of one must not leak into the other), one in a gap no read reaches,
    one before every read, one behind every read, and one whose range is the batch's last read (no read to stop at: hi == n)"""
    reads = V.seeded_batch(7, 200, start=3000, step=(0, 2), ops="MMMMMIDS")
    last = (8000, [("M", 30)], "ACGT" * 7 + "AC", [30] * 30)
    reads = reads + [last]
    rng = random.Random(7)
    rows = sorted(V.random_sites(rng, reads[50], 20, 4) + V.random_sites(rng, reads[60], 20, 4))
    rows += [(6000, "A", "C"), (10, "A", "C"), (9000, "A", "C"), (8005, "C", "G"), (8010, "GT", "G")]
    n = len(rows)
    nbhd = [(0, n - 5), (2, n - 6), (n - 5, n - 4), (n - 4, n - 3), (n - 3, n - 2), (n - 2, n)]
    got = three_way(torch_cuda, caller, reads, rows, nbhd)
    assert list(got["info"]["n_reads_used"][2:5]) == [0, 0, 0] and int(got["info"]["n_reads_used"][5]) == 1
    assert int(got["groups"]["first_read"][-1]) == len(reads) - 1


@pytest.mark.parametrize("n_reads", [64, 1000])
def test_all_veads_equal(torch_cuda, caller, n_reads):
    """one group of n: every lane of every wave contends for one slot, and the representative must still be the first read"""
    reads = [(4000, [("M", 50)], "ACGTA" * 10, [30] * 50)] * n_reads
    got = three_way(torch_cuda, caller, reads, [(4005 + 3 * i, "C", "T") for i in range(10)], [(0, 10)])
    assert len(got["groups"]) == 1 and tuple(got["groups"][0])[:3] == (0, 0, n_reads)


def test_all_veads_distinct(torch_cuda, caller):
    """n groups of one: 1024 reads that spell their own index in 10 two-allele sites; the table holds twice the pairs and never fills, the
    groups come out in read order whichever wave ran first"""
    n = 1024
    rows = [(4005 + 3 * i, "A", "C") for i in range(10)]
    reads = []
    for k in range(n):
        b = ["G"] * 50
        for i in range(10):
            b[5 + 3 * i] = "C" if (k >> i) & 1 else "A"
        reads.append((4000, [("M", 50)], "".join(b), [30] * 50))
    perm = list(range(n))
    random.Random(3).shuffle(perm)
    reads = [reads[k] for k in perm]
    got = three_way(torch_cuda, caller, reads, rows, [(0, 10)])
    assert list(got["groups"]["first_read"]) == list(range(n)) and set(got["groups"]["n_veads"]) == {1}


def test_clipped_then_skipped_and_the_stopping_read(torch_cuda, caller):
    """a read that counts as clipped and is then skipped (2M2S ending one base before the first site), and a zero-span read at the
    look-ahead + 1 that the scan stops at and still clip-tests"""
    rows = [(10, "A", "C")]
    reads = [(8, V.parse_cigar("2M2S"), "ACGT", [30] * 4), (12, V.parse_cigar("2I2S"), "ACGT", [30] * 4), (12, V.parse_cigar("4M"), "ACGT", [30] * 4)]
    got = three_way(torch_cuda, caller, reads, rows, [(0, 1)])
    assert (int(got["info"]["n_clipped_reads"][0]), int(got["info"]["n_reads_used"][0]), len(got["groups"])) == (2, 0, 0)


def test_short_capacities_and_the_same_call_twice(torch_cuda, caller):
    """one short of each capacity: only the counts; the right sizes: everything; the same call again: identical bytes"""
    reads = V.seeded_batch(11, 150, start=3000, step=(0, 1), ops="MMMMMIDS")
    rng = random.Random(11)
    rows = sorted(V.random_sites(rng, reads[70], 20, 6))
    batch = device_batch(reads)
    full = device_groups(torch_cuda, caller, batch, rows, [(0, 6), (1, 5)])
    ng, ns, _ = full["n_out"]
    assert ng > 2
    for caps in ((ng - 1, ns), (ng, ns - 1)):
        raw = run_device(torch_cuda, caller, batch, rows, [(0, 6), (1, 5)], caps)
        assert tuple(int(v) for v in raw["n_out"]) == (ng, ns, 0)
        assert (raw["groups"] == SENTINEL).all() and (raw["states"] == SENTINEL).all()
    a = run_device(torch_cuda, caller, batch, rows, [(0, 6), (1, 5)], (ng, ns))
    b = run_device(torch_cuda, caller, batch, rows, [(0, 6), (1, 5)], (ng, ns))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    V.assert_same(full, V.statement(reads, rows, [(0, 6), (1, 5)]))


def test_unsorted_positions_are_refused_with_the_first_offender(torch_cuda, caller):
    reads = V.seeded_batch(5, 300, start=3000, step=(1, 2))
    for bad in (200, 130):   # the lower one wins, whichever wave sees its own first
        p, cigar, b, q = reads[bad]
        reads[bad] = (reads[bad - 1][0] - 1, cigar, b, q)
    with pytest.raises(PiscesHipError) as e:
        run_device(torch_cuda, caller, device_batch(reads), [(3100, "A", "C")], [(0, 1)], (16, 16))
    assert e.value.code == _abi.E_INVALID_ARG and e.value.message.endswith("not sorted by position at read 130")


@pytest.fixture(scope="module")
def chr21():
    z = np.load(os.path.join(V.GOLDEN, "bam_scylla_chr21.npz"))
    rows = [(int(p), str(r), str(a)) for p, r, a in zip(z["vcf_position"], z["vcf_ref"], z["vcf_alt"])]
    return z, rows, V.chain(rows, 50) + [(i, i + 1) for i in range(len(rows))]


def test_chr21_bam_bytes_decoded_on_the_device(torch_cuda, chr21):
    """BAM bytes in, phasing evidence out: the reference's Scylla BAM through pisces_hip_bam_decode, the vead pass over the handle's
    decoded batch (device_batch = NULL) == the statement on bam_fetch() of the same decode; then the fetched arrays uploaded and passed as
    an explicit device batch.  The decode's own state is left alone: the batch can still be fetched and added afterwards."""
    from pisces_amd import engine
    z, rows, nbhd = chr21
    with engine.HipVariantCaller(_abi.default_config()) as c:
        counts = c.bam_decode(z["bam"], int(z["ref_id"]), min_map_quality=0, skip_duplicates=False)
        fetched = c.bam_fetch()
        reads = V.reads_of(fetched)
        assert counts["reads"] == len(reads) == len(z["position"])   # every mapped, primary record with a CIGAR: the fixture's own reads
        assert all(fetched[k].tobytes() == np.ascontiguousarray(z[k]).tobytes() for k in ("position", "cigar_op", "cigar_len", "bases", "quals"))
        want = V.statement(reads, rows, nbhd)
        got = device_groups(torch_cuda, c, None, rows, nbhd)
        V.assert_same(got, want, "decoded batch")
        assert len(got["groups"]) > 100 and got["info"]["n_clipped_reads"].max() > 0
        again = c.bam_fetch()
        assert all(fetched[k].tobytes() == again[k].tobytes() for k in fetched)
        explicit = device_groups(torch_cuda, c, device_batch(fetched), rows, nbhd)
        V.assert_same(explicit, want, "explicit device batch")
        c.AddDecodedReads()
        # a batch whose arrays went into the read store is gone (PISCES_E_STATE); one that was copied there is still the decoded batch
        try:
            V.assert_same(device_groups(torch_cuda, c, None, rows, nbhd), want, "after the add")
        except PiscesHipError as e:
            assert e.code == _abi.E_STATE and "added to the read store" in e.message
    with engine.HipVariantCaller(_abi.default_config()) as c:
        with pytest.raises(PiscesHipError) as e:
            run_device(torch_cuda, c, None, rows, nbhd, (0, 0))
        assert e.value.code == _abi.E_STATE and "no decoded batch" in e.value.message


def test_a_handle_that_ran_the_pass_still_calls_the_committed_fixture(torch_cuda):
    """the pass leaves the handle's state alone: the oracle's rows for synthetic_small.npz afterwards"""
    from pisces_amd import engine
    from tests.test_gpu_parity import assert_records_match
    z = np.load(os.path.join(V.GOLDEN, "synthetic_small.npz"))
    exp = z["expected"].view(_abi.CALLED_ALLELE_DTYPE)
    reads = V.seeded_batch(2, 100, start=3000, step=(0, 1))
    with engine.HipVariantCaller(_abi.default_config()) as c:
        three_way(torch_cuda, c, reads, [(3050, "A", "C"), (3052, "AC", "A")], [(0, 2)])
        c.SetReference(z["ref"])
        c.AddObservations(z["positions"], z["tuples"])
        got = c.Call(None)
    assert_records_match(got, exp)
