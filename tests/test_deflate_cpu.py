"""What tests/deflate_synth.py writes, held to zlib and to its own tracer on the CPU: every positive member of families A-D and F is a
stream zlib accepts, decodes to what the builder meant, and sits in the file where the builder's block table says; and the decoder
regimes the families exist for are PROVED to be reached, from the tracer's events and the group geometry (deflate_synth.group_offset)
alone, before tests/test_deflate_gpu.py runs the same files through bgzf_inflate_kernel.  Family E's rows are all refused by zlib."""
import functools
from collections import Counter

import pytest

from pisces_amd import engine
from tests import deflate_synth as ds

FAMILIES = {"A": ds.family_a, "B": ds.family_b, "C": ds.family_c, "D": ds.family_d, "F": ds.family_f}
ALL64 = set(range(64))


def files_of(name):
    f = FAMILIES[name]()
    return f if isinstance(f, list) else [f]


@functools.lru_cache(None)
def traces(name):
    """[(member, Trace)] of a family"""
    return [(m, ds.trace(m.payload, m.in_offset)) for f in files_of(name) for m in f.members]


def by_name(name):
    return {m.name: (m, t) for m, t in traces(name)}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_member_is_accepted_by_zlib_and_means_what_the_builder_meant(name):
    n = 0
    for f in files_of(name):
        blocks, total = engine.bgzf_scan(f.data)
        assert [(b.in_offset, b.in_length, b.out_offset, b.out_length, b.crc32) for b in blocks] == f.table and total == f.table[-1][2]
        for m in f.members:
            assert f.data[m.in_offset:m.in_offset + len(m.payload)] == m.payload and (m.phase is None or m.in_offset % 16 == m.phase)
            out, eof = ds.zlib_inflate(m.payload)
            assert eof and out == m.data, m.name
            n += 1
    for m, t in traces(name):
        assert t.out == m.data and t.end_bit <= 8 * len(m.payload), m.name
    assert n == len(traces(name)) and n == {"A": 4, "F": ds.F_MEMBERS}.get(name, n)


# ---------------------------------------------------------------- A
def test_family_a_puts_every_construct_at_every_group_offset():
    hits = Counter()    # (construct, offset)
    t_short, t_long = set(), set()
    for m, t in traces("A"):
        for e in t.events:
            off = ds.group_offset(m.in_offset, e.bit)
            if e.kind == "literal":
                hits[("literal", e.code_len), off] += 1
            elif e.kind == "eob":
                hits[("eob", e.code_len), off] += 1
            elif e.kind == "length":
                hits[("length", e.code_len, e.len_extra), off] += 1
                hits[("distance", e.dist_code_len, e.dist_extra), ds.group_offset(m.in_offset, e.dist_bit)] += 1
                start = off + e.dist_bit - e.bit    # the kernel's `t`: 64 and more = the distance code starts in the next group
                assert start == off + e.code_len + e.len_extra
                (t_short if e.code_len <= ds.LEN_LUT_BITS else t_long).add(start)
    constructs = [("literal", b) for b in (2, 3, 9, 10, 11, 15)] + [("eob", b) for b in ds.A_EOB] + \
        [("length", b, x) for b, x in ds.A_LENGTHS] + [("distance", b, x) for b, x in ds.A_DISTANCES]
    assert len(constructs) == 20
    for c in constructs:
        assert {off for (cc, off) in hits if cc == c} == ALL64, c
    assert any(b <= ds.LEN_LUT_BITS for b, _ in ds.A_LENGTHS) and any(b > ds.LEN_LUT_BITS for b, _ in ds.A_LENGTHS)
    assert any(b <= ds.DIST_LUT_BITS for b, _ in ds.A_DISTANCES) and any(b > ds.DIST_LUT_BITS for b, _ in ds.A_DISTANCES)
    # the distance code of a short-coded length starts at every offset up to 63 + 10 + 5, of a long-coded one up to 63 + 15 + 5
    # (from the shortest length code on: nothing starts a distance code before the length code in front of it has ended)
    assert t_short == set(range(4, 79)) and t_long == set(range(11, 84))
    print("family A: %d constructs x 64 offsets, %d hits, fewest per cell %d" % (len(constructs), sum(hits.values()), min(hits.values())))


# ---------------------------------------------------------------- B
def test_family_b_reaches_the_code_shapes_it_names():
    b = by_name("B")
    blocks = lambda name: b[name][1].blocks
    events = lambda name: b[name][1].events
    for name in ("B/single_distance_code", "B/single_distance_code_symbol4"):
        assert [k["n_dl"] for k in blocks(name)] == [1] and sum(e.kind == "length" for e in events(name)) == 2
    for name, at in (("B/eob_only_first", 0), ("B/eob_only_middle", 1), ("B/eob_only_last", 2)):
        assert [k["n_ll"] == 1 for k in blocks(name)] == [i == at for i in range(3)] and blocks(name)[at]["n_dl"] == 0
    assert [(k["n_ll"], k["n_dl"]) for k in blocks("B/eob_only_alone")] == [(1, 0)] and b["B/eob_only_alone"][0].data == b""
    assert blocks("B/no_distance_code")[0]["n_dl"] == 0 and len(events("B/no_distance_code")) == 5
    k = blocks("B/minimal_header")[0]
    assert (k["nlen"], k["ndist"], k["ncode"]) == (257, 1, 5)    # (HCLEN 4 cannot announce an end-of-block code: family E)
    k = blocks("B/maximal_header")[0]
    assert (k["nlen"], k["ndist"], k["ncode"]) == (286, 30, 19) and k["cl"][15] > 0
    k = blocks("B/repeat16_after_first_length")[0]
    assert k["rle"][0][0] == 16 and k["rle"][0][2] == 1
    k = blocks("B/repeat16_into_distance_lengths")[0]
    assert any(s == 16 and at < k["nlen"] < at + rep for s, rep, at in k["rle"])
    k = blocks("B/repeat17_18_extremes_and_exact_end")[0]
    assert {(17, 3), (17, 10), (18, 11), (18, 138)} <= {(s, rep) for s, rep, _ in k["rle"]}
    s, rep, at = k["rle"][-1]
    assert s == 18 and at + rep == k["nlen"] + k["ndist"]
    k = blocks("B/deep_codes")[0]
    assert (k["max_ll"], k["max_dl"]) == (15, 15)
    assert {15} <= {e.code_len for e in events("B/deep_codes") if e.kind == "literal"} and {15} <= {e.code_len for e in events("B/deep_codes") if e.kind == "length"}
    assert {14, 15} <= {e.dist_code_len for e in events("B/deep_codes") if e.kind == "length"}
    assert any(e.kind == "eob" and e.code_len == 14 for e in events("B/deep_codes"))
    # every length and distance symbol at both ends of its extra bits, in a dynamic and in a fixed block
    want_len = {(257 + i, x) for i in range(29) for x in (0, (1 << ds.LEN_EXTRA[i]) - 1)}
    want_dist = {(i, x) for i in range(30) for x in (0, (1 << ds.DIST_EXTRA[i]) - 1)}
    for name, kind in (("B/all_symbols_dynamic", "dynamic"), ("B/all_symbols_fixed", "fixed")):
        pairs = [e for e in events(name) if e.kind == "length"]
        assert blocks(name)[1]["kind"] == kind and events(name)[0].kind == "stored" and events(name)[0].length == 32768
        assert {(e.sym, e.length - ds.LEN_BASE[e.sym - 257]) for e in pairs} == want_len
        assert {(e.dist_sym, e.distance - ds.DIST_BASE[e.dist_sym]) for e in pairs} == want_dist
        assert {e.sym for e in pairs if e.length == 258} == {284, 285} and max(e.distance for e in pairs) == 32768
    assert {e.code_len for e in events("B/all_symbols_fixed") if e.kind != "stored"} == {7, 8, 9}
    assert {e.code_len for e in events("B/all_symbols_fixed") if e.kind == "literal"} == {8, 9}
    assert {e.code_len for e in events("B/all_symbols_fixed") if e.kind == "length"} == {7, 8}


# ---------------------------------------------------------------- C
def test_family_c_reaches_the_block_transitions_it_names():
    c = traces("C")
    kinds = ("stored", "fixed", "dynamic")
    seen = {(t.blocks[0]["kind"], t.blocks[1]["kind"], t.blocks[1]["header_bit"] % 8) for m, t in c if "pair" in m.info}
    # behind a stored block a header can only start on a byte boundary; behind a fixed or dynamic block it starts at every bit of a byte
    assert seen == {(a, b, k) for a in kinds for b in kinds for k in (range(8) if a != "stored" else (0,))}
    first_stored = [(m, t.events[0]) for m, t in c if m.name.startswith("C/stored/residue")]
    assert all(e.kind == "stored" for _, e in first_stored)
    assert {((m.in_offset + e.bit // 8) % 16, e.length) for m, e in first_stored} == {(r, n) for r in range(16) for n in ds.C_STORED_SIZES}
    assert {(m.in_offset + e.bit // 8 + e.length) % 4 for m, e in first_stored} == {0, 1, 2, 3}    # inflate_seek's skew behind the data
    assert {(m.in_offset + e.bit // 8 + e.length) % 16 for m, e in first_stored} == set(range(16))
    largest = [t for m, t in c if m.name == "C/stored/largest"][0]
    assert largest.events[0].length == ds.C_LARGEST_STORED and len(ds.bgzf_member(b"\0" * (ds.C_LARGEST_STORED + 5), 0, 0)) == 65536
    for kind in ("stored", "fixed", "dynamic", "dynamic_eob_only"):
        m, t = [x for x in c if x[0].name == "C/empty200/" + kind][0]
        assert len(t.blocks) == 201 and all(k["kind"] == kind.split("_")[0] for k in t.blocks[:200]) and len(m.data) == 8
        assert all(e.out_pos == 0 and e.kind in ("eob", "stored") and not e.length for e in t.events if e.block < 200)
    reach = set()
    for m, t in c:
        if "reach" in m.info:
            e = [e for e in t.events if e.block == 1][0]
            assert e.kind == "length" and e.out_pos == 7
            reach.add((t.blocks[0]["kind"], t.blocks[1]["kind"], e.out_pos - e.distance))
    assert reach == {(a, b, d) for a in kinds for b in kinds[1:] for d in (0, 1)}
    assert sorted(8 * len(m.payload) - t.end_bit for m, t in c if m.name.startswith("C/final_eob/")) == list(range(8))
    assert sorted(len(m.payload) - (t.end_bit + 7) // 8 for m, t in c if "trailing" in m.info) == sorted(ds.C_TRAILING)


# ---------------------------------------------------------------- D
def test_family_d_groups_hold_what_each_case_claims():
    n = 0
    names = set()
    for m, t in traces("D"):
        claim = m.info["claim"]
        assert ds.group_offset(m.in_offset, claim["bit"]) == 0
        g = ds.group_bit(m.in_offset, claim["bit"]) // 64
        group = [e for e in t.events if ds.group_bit(m.in_offset, e.bit) // 64 == g]
        # short codes only: nothing but the end-of-block code stops the walk, so a group is written in one piece
        assert all(e.code_len <= ds.LEN_LUT_BITS and (e.kind != "length" or e.dist_code_len <= ds.DIST_LUT_BITS) for e in t.events if e.kind != "stored")
        pairs = [e for e in group if e.kind == "length"]
        first = group[0].out_pos
        assert len(pairs) == claim["pairs"] and sum(e.length for e in pairs) == claim["pair_bytes"], m.name
        if pairs:
            assert max(e.out_pos - e.distance + e.length for e in pairs) - first == claim["reach"], m.name
        if "lits" in claim:
            assert sum(e.kind == "literal" for e in group) == claim["lits"], m.name
        if m.name.endswith("/ends_in_group"):
            assert group[-1].kind == "eob" and group[-1].out_pos == len(m.data), m.name
        else:
            assert all(e.kind != "eob" for e in group)
        names.add(m.name.split("/")[1])
        n += 1
    assert n == 2 * len(names) and names == {s[0] for s in ds.D_SHAPES} | {"pairs32"}
    claims = {m.name[2:]: m.info["claim"] for m, _ in traces("D")}
    assert claims["lit64"]["lits"] == 64 and (claims["pairs32"]["pairs"], claims["pairs32"]["pair_bytes"]) == (32, 96)
    assert [claims[f"pair_bytes{k}"]["pair_bytes"] for k in (63, 64, 65)] == [63, 64, 65] and all(claims[f"pair_bytes{k}"]["reach"] <= 0 for k in (63, 64, 65))
    assert [claims[k]["reach"] for k in ("source_ends_at_group_start", "source_ends_one_past_group_start", "source_ends_at_group_start_behind_literals",
                                         "source_ends_one_past_behind_literals", "source_is_literal_of_the_group")] == [0, 1, 0, 1, 3]


# ---------------------------------------------------------------- E
def test_family_e_is_refused_by_the_reference_row_by_row():
    rows = ds.family_e()
    assert len({r.name for r in rows}) == len(rows)
    for r in rows:
        assert not r.accept and not ds.reference_verdict(r.payload, r.isize), r.name
        assert r.status in (None, 2, 3, 4, 5, 6, 7, 8)
        f = ds.negative_file(r)
        assert [ds.reference_verdict(m.payload, f.table[i][3]) for i, m in enumerate(f.members)] == [True, False, True]
    assert Counter(r.status for r in rows) == {None: 1, 2: 1, 3: 1, 4: 14, 5: 8, 6: 3, 7: 4, 8: 1}
    # an ISIZE one off is the whole defect of the status 7 and 8 rows: their streams are valid
    for r in rows:
        if r.status in (7, 8):
            out, eof = ds.zlib_inflate(r.payload)
            assert eof and len(out) == r.isize + (1 if r.status == 7 else -1)


# ---------------------------------------------------------------- F
def test_family_f_histogram_of_regimes():
    h = Counter()
    for m, t in traces("F"):
        for k in t.blocks:
            h["blocks " + k["kind"]] += 1
            if k["kind"] == "dynamic":
                h["single literal/length code"] += k["n_ll"] == 1
                h["single distance code"] += k["n_dl"] == 1
                h["no distance code"] += k["n_dl"] == 0
                h["15-bit literal/length code"] += k["max_ll"] == 15
                h["15-bit distance code"] += k["max_dl"] == 15
        for e in t.events:
            h[e.kind] += 1
            if e.kind == "literal":
                h["long literal codes"] += e.code_len > ds.LEN_LUT_BITS
            elif e.kind == "eob":
                h["long end-of-block codes"] += e.code_len > ds.LEN_LUT_BITS
            elif e.kind == "length":
                h["long length codes"] += e.code_len > ds.LEN_LUT_BITS
                h["long distance codes"] += e.dist_code_len > ds.DIST_LUT_BITS
                h["t >= 64"] += ds.group_offset(m.in_offset, e.bit) + e.dist_bit - e.bit >= 64
                h["self-overlapping pairs"] += e.distance < e.length
                h["length 258 as 284 + 31"] += e.sym == 284 and e.length == 258
        h["members"] += 1
        h["empty members"] += not m.data
    print("family F regimes:", ", ".join(f"{k} {v}" for k, v in sorted(h.items())))
    assert h["members"] == ds.F_MEMBERS
    for k in ("long literal codes", "long length codes", "long distance codes", "long end-of-block codes", "t >= 64", "single literal/length code",
              "single distance code", "no distance code", "blocks stored", "blocks fixed", "blocks dynamic", "self-overlapping pairs",
              "15-bit literal/length code", "15-bit distance code", "length 258 as 284 + 31", "empty members"):
        assert h[k] >= 1, k    # reached at all is the condition; the printed counts say how often
