"""The read store's geometry grid on the CPU (tests/store_geometry.py): the constants come from the kernel source, the two references
(a numpy statement of AddAlleleCounts from the reference's C#, and the oracle) agree cell by cell before either judges the device, the
oracle's rows show every count the tensor holds but the ones named below, and the grid reaches every required regime of the model from
at least two independent cases.
"""
import collections
import re

import numpy as np

from pisces_amd import _abi
from tests import store_geometry as sg

K = sg.K


def test_constants_come_from_the_source():
    assert (K.tile, K.half, K.block, K.unit, K.sub_chunk) == (64, 32, 64, 16, 16)
    assert K.pair_slots == 2 * K.block + 2 * K.unit and K.segment_pad >= K.half + K.lane_bytes - 1
    assert K.span_max == K.delta_max == 0xFFFF and K.desc_len_mask == 0xFFFFF and K.grid_gap_cells == 65536
    assert K.waves == sg.WAVES and K.max_segments == 8
    assert [sg.waves_for(n, 256) for n in (1, 256, 257, 768, 769, 8192, 8193)] == [16, 16, 4, 4, 2, 2, 1]
    # a source with other numbers moves the constants: nothing here is a copy of them
    st = sg._source("store_kernels.hip.h")
    k2 = sg.parse_constants(store_text=re.sub(r"(constexpr int kGridGapCells = )\d+", r"\g<1>4096", st))
    assert k2.grid_gap_cells == 4096
    k3 = sg.parse_constants(surface_text=sg._source("surface_store.inc.h").replace("(int64_t)h->n_cus * 32 ? 2 : 1", "(int64_t)h->n_cus * 16 ? 2 : 1"))
    assert sg.waves_for(8192, 256, k3) == 1
    # a segment whose gaps the smaller grid does not fill goes to the search in the model too
    reach = sg.scene_named("reach")
    assert sg.Segment(reach.batches[0], k=K).grid_usable and not sg.Segment(reach.batches[1], k=K).grid_usable
    far_gap = sg.Segment([dict(reach.batches[0][0], pos=100), dict(reach.batches[0][0], pos=100 + 5000)], k=K)
    assert far_gap.grid_usable and not sg.Segment(far_gap.reads, k=k2).grid_usable


def test_the_model_accounts_for_every_fragment_once():
    """Every fragment of a tile's range is in exactly one block, every block in exactly one wave, a block's pairs fit the LDS list, a
    unit load stays inside the pad around a segment's bytes, and the composition cases have the compositions they are named for."""
    for scene in sg.build_scenes():
        for mode in ("own", "appended"):
            for fl in sg.flushes_of(scene, mode):
                for g, (nf, floor) in zip(fl.segments, fl.floors):
                    for ts, _ in sg.tile_starts(fl.keys[:3]):
                        m = sg.tile_model(sg._refloored(g, nf, floor), ts)
                        assert sum(b.count for b in m.blocks) == len(m.idx) and all(0 < b.count <= K.block for b in m.blocks)
                        for b in m.blocks:
                            assert K.unit * b.ul + b.nr + K.unit <= K.pair_slots and b.nl + K.unit <= K.pair_slots
                        for nw in K.waves:
                            assert sorted(x for w in range(nw) for x in range(w, len(m.blocks), nw)) == list(range(len(m.blocks)))
    blocks = sg.scene_named("blocks")
    g = sg.Segment(blocks.batches[0])
    for name, lo, _ in blocks.cases:
        if name.startswith("composition"):
            nl, nr = (int(x) for x in re.findall(r"\d+", name))
            b0 = sg.tile_model(g, lo + 3 * K.tile).blocks[0]
            assert (b0.nl, b0.nr) == (nl, nr), (name, b0.nl, b0.nr)
        if name.startswith("range of"):
            n = int(re.findall(r"\d+", name)[0])
            assert len(sg.tile_model(g, lo + 7 * K.tile).idx) == n, name
    # the floor scenes: the floored fragments are no multiple of 64, so a block of 64 holds both kinds
    for n in (2, 3):
        fl = sg.flushes_of(sg.scene_named("floor, %d flushes in a row" % n), "appended")
        assert len(fl) == n + 1 and all(nf % K.block != 0 for f in fl[1:] for nf, _ in f.floors)
        assert [f.floors[0][1] for f in fl] == [0] + [sg.BLOCK * (2 + i) + 1 for i in range(n)]
    # the search's rounds at the segment sizes the grid names
    search = sg.scene_named("search")
    rounds = {len(sg.Segment(b).pos0): sg.Segment(b).range_of(sg.tile_at(2 + i, 9)) for i, b in enumerate(search.batches[:len(sg.SEGMENT_SIZES)])}
    assert {n: (r.method, r.rounds) for n, r in rounds.items()} == {1: ("grid", 0), 31: ("search", 1), 32: ("search", 1), 33: ("search", 2),
                                                                  1024: ("search", 2), 1025: ("search", 2), 1057: ("search", 3)}


def test_the_two_references_agree_cell_by_cell():
    """count_tensor (numpy, from RegionStateManager.cs) == orc.State.add_allele_counts over every block a scene touches."""
    cells = 0
    for scene in sg.build_scenes():
        for start, n in sg.runs_of_keys(scene.keys):
            a = sg.count_tensor(scene.reads, start, n, scene.min_bq)
            b = sg.oracle_tensor(scene.reads, start, n, scene.min_bq)
            if not (a == b).all():
                first = np.argwhere(a != b)[0]
                raise AssertionError("%s: %d cells differ; first [locus %d][allele %d][direction %d][anchor %d]: numpy %d, oracle %d; %s" % (
                    scene.name, int((a != b).sum()), start + first[0], first[1], first[2], first[3], a[tuple(first)], b[tuple(first)],
                    sg.describe_locus(scene, int(start + first[0]))))
            assert a.sum() > 0
            cells += a.size
    assert cells > 10_000_000


def point_rows(rows):
    cat = _abi.info_category(rows["info"].astype(np.int64))
    return rows[(cat == _abi.CAT_SNV) | (cat == _abi.CAT_REFERENCE)]


def test_the_oracles_rows_show_the_tensor():
    """Under both configurations the Reference and SNV rows of the oracle equal the tensor folded over anchors (coverage and support by
    direction, no-calls, reference support).  Under "every allele a row" every locus with coverage has a row, every allele with a count
    other than the reference's has its own row, and at every locus reference support + the SNV rows' supports + the deleted positions'
    count is the coverage: a base moved to another row or another locus changes an integer of some record.

    What the rows cannot show, and GetCounts carries instead: the anchor bin of any count (the rows fold the bins); the split of a
    locus' deletion count from its reference count by direction where an SNV row is there (the rows give their sum by direction and the
    reference support in all); and the counts of a locus on which an insertion or deletion row stands and no SNV row does (the locus
    before a gap: the reference's caller emits no Reference row next to a variant, and the indel row's coverage is the mean of two loci)."""
    for scene in sg.build_scenes():
        if scene.name in sg.NO_ORACLE_ROWS:
            continue
        tensor = sg.count_tensor(scene.reads, 1, scene.n_loci, scene.min_bq)
        folded = tensor.sum(axis=3, dtype=np.int64)
        cov = folded[:, [0, 1, 2, 3, 5], :].sum(axis=(1, 2))
        for which in sg.CONFIGS:
            rows, _ = sg.oracle_rows(scene, which)
            pr = point_rows(rows)
            assert len(pr) and sg.rows_agree_with_tensor(pr, tensor, scene.ref) > 9 * len(pr), (scene.name, which)
            if which != "every allele a row":
                continue
            li = pr["position"].astype(np.int64) - 1
            any_count = folded.sum(axis=(1, 2)) > 0
            cat = _abi.info_category(rows["info"].astype(np.int64))
            indel_loci = set((rows["position"][(cat != _abi.CAT_SNV) & (cat != _abi.CAT_REFERENCE)].astype(np.int64) - 1).tolist())
            hidden = set(np.flatnonzero(any_count).tolist()) - set(li.tolist())
            assert set(li.tolist()) <= set(np.flatnonzero(any_count).tolist()) and hidden <= indel_loci and len(hidden) <= 40, (scene.name, sorted(hidden)[:10])
            cov = np.where(np.isin(np.arange(scene.n_loci), li), cov, 0)              # (from here on: the loci that have a point row)
            info = pr["info"].astype(np.int64)
            alt, rt = _abi.info_alt(info), _abi.info_ref(info)
            snv = _abi.info_category(info) == _abi.CAT_SNV
            shown = np.zeros(scene.n_loci, np.int64)
            np.add.at(shown, li[snv], pr["allele_support"][snv])
            ref_support = np.zeros(scene.n_loci, np.int64)
            ref_support[li] = pr["reference_support"]
            total = np.zeros(scene.n_loci, np.int64)
            total[li] = pr["total_coverage"]
            deleted = folded[:, 5, :].sum(axis=1)
            on = np.isin(np.arange(scene.n_loci), li)
            np.testing.assert_array_equal((ref_support + shown + deleted)[on], total[on], err_msg=scene.name)
            np.testing.assert_array_equal(total[on], cov[on], err_msg=scene.name)
            # every non-reference base with a count has its row
            letters = np.frombuffer(b"AGCT", np.uint8)
            ref_allele = np.searchsorted(np.sort(letters), scene.ref[:scene.n_loci])          # index into sorted "ACGT"
            ref_allele = np.array([0, 2, 1, 3])[ref_allele]                                    # -> AlleleType A G C T
            counted = folded[:, :4, :].sum(axis=2) > 0
            counted[np.arange(scene.n_loci), ref_allele] = False
            has_row = np.zeros((scene.n_loci, 4), bool)
            has_row[li[snv], alt[snv]] = True
            assert (has_row[on] == counted[on]).all(), scene.name
            assert (rt[snv] == ref_allele[li[snv]]).all()


def regime_table():
    table = collections.defaultdict(set)
    for scene in sg.build_scenes():
        for mode in ("own", "appended"):
            for reg, who in sg.scene_regimes(scene, mode).items():
                table[reg] |= who
    return table


def test_the_grid_reaches_every_required_regime_twice():
    table = regime_table()
    req = sg.required_regimes()
    assert len(set(req)) == len(req) >= 120 and sg.UNREACHED == []
    short = [(r, sorted(table.get(r, ()))) for r in req if len(table.get(r, ())) < 2 and r not in sg.UNREACHED]
    groups = collections.defaultdict(list)
    for r in req:
        groups[r[0] if r[0] not in ("block", "range") else r[0] + " " + r[1]].append(len(table.get(r, ())))
    lines = ["%-28s %3d regimes, cases per regime %d .. %d" % (g, len(v), min(v), max(v)) for g, v in sorted(groups.items())]
    print("\n".join(lines))
    print("regimes the model names over the grid: %d" % len(table))
    assert not short, "required regimes reached by fewer than two independent cases:\n%s\n%s" % ("\n".join("%s: %s" % x for x in short), "\n".join(lines))
    # the same with tiles of 59, 48 and 33 loci: the exhaustive (pr, er) edges stay exhaustive whatever the tile size
    for tl in (59, 48, 33):
        masks = set()
        for name in ("edges", "edges, per-base directions"):
            masks |= {r for r in sg.scene_regimes(sg.scene_named(name), "own", tl) if r[0] == "mask"}
        assert {("mask", a, e) for a in range(9) for e in range(9) if a < e} <= masks, tl


def test_the_scenes_are_what_they_say():
    scenes = {s.name: s for s in sg.build_scenes()}
    assert len(scenes) == 17
    for s in scenes.values():
        assert len(s.batches) <= 9 and len(s.ups) == len(s.batches) and sum(len(b) for b in s.batches) == len(s.reads) < 7000
        assert all(rd["pos"] >= 1 and sum(l for o, l in rd["cigar"] if o in sg.READ_OPS) == len(rd["seq"]) == len(rd["quals"]) for rd in s.reads)
    for name in ("edges", "blocks", "deletions"):
        a, b = scenes[name], scenes[name + ", per-base directions"]
        assert all("dirs" not in rd for rd in a.reads) and all(len(rd["dirs"]) == len(rd["seq"]) for rd in b.reads)
        assert [rd["seq"] for rd in a.reads] != [rd["seq"] for rd in b.reads]               # drawn apart
    edges = scenes["edges"]
    for _, key, j in sg.EDGE_TILES:
        s = sg.tile_at(key, j)
        got = {(rd["pos"] - s, rd["pos"] - s + rd["cigar"][0][1]) for rd in edges.reads if s <= rd["pos"] and rd["pos"] + rd["cigar"][0][1] <= s + K.tile}
        assert {(a, e) for a in range(K.tile) for e in range(a + 1, K.tile + 1)} <= got
    assert sum(1 for a, e in ((a, e) for a in range(64) for e in range(a + 1, 65))) == 2080
    batches = scenes["batches"]
    assert len(batches.batches) == 9 > K.max_segments and all(b == sorted(b, key=lambda r: r["pos"]) for b in batches.batches)
    assert not sg.Segment(batches.reads).sorted
    for s in (scenes["floor, 2 flushes in a row"], scenes["floor, 3 flushes in a row"]):
        for b, (batch, up) in enumerate(zip(s.batches[:-1], s.ups)):
            cuts = {up + 1 - rd["pos"] for rd in batch if rd["pos"] <= up < rd["pos"] + sg.ref_span_of(rd["cigar"]) - 1 and len(rd["cigar"]) == 1}
            assert set(range(1, 201)) <= cuts
            assert all(rd["pos"] > up for later in s.batches[b + 1:] for rd in later)          # nothing is added into a flushed block
    fields = scenes["fields by N"].reads + scenes["fields by D"].reads
    assert {sg.ref_span_of(rd["cigar"]) for rd in fields} >= {0xFFFE, 0xFFFF, 0x10000, 0x10001}
    assert sum(sg.shape_read(rd)[0].generic for rd in fields) == 8 and {rd["cigar"][1][0] for rd in fields} == {"N", "D"}
    dele = scenes["deletions"]
    g = sg.Segment(dele.reads)
    lo = next(lo for name, lo, _ in dele.cases if name.startswith("more than 128"))
    m = sg.tile_model(g, lo + 5 * K.tile)
    assert (m.kind == 1).sum() > 128
    shapes = {sg.cigar_string(rd["cigar"]): sg.shape_read(rd)[0] for rd in dele.reads}
    assert shapes["10M2D3N10M"].why == ("gap chain",) and shapes["10M2D2I3D10M"].why == ("gap chain",) and not shapes["10M2D1M3D10M"].generic


def test_late_reads_count_as_done_processing_says():
    """The late-reads scene's reference, from the oracle's own state machine: add the first batch, DoneProcessing up to the flushed edge,
    add the late batch.  Its counts equal late_tensor, cell by cell."""
    from tests import orc
    scene = sg.late_scene()
    n = 3 * sg.BLOCK
    st = orc.State(1, n, min_bq=scene.min_bq)
    st.track_blocks(sg.BLOCK)
    add = lambda rd: st.add_allele_counts(orc.make_read(rd["pos"], rd["seq"], cigar=rd["cigar"], quals=rd["quals"], reverse=rd["reverse"], dirs=rd.get("dirs")))
    assert all(add(rd) == 0 for rd in scene.batches[0])
    st.done_processing(scene.ups[0])
    assert not st.counts()[:scene.ups[0]].any() and st.counts()[scene.ups[0]:].any()
    assert all(add(rd) == 0 for rd in scene.batches[1])
    want = sg.late_tensor(scene, n)
    np.testing.assert_array_equal(st.counts(), want)
    below = want[:scene.ups[0]].sum()
    assert 0 < below < sg.count_tensor(scene.reads, 1, n)[:scene.ups[0]].sum()
