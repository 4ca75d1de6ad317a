"""The tuple path at every segment geometry: infrastructure of tests/test_tuple_geometry_cpu.py and tests/test_tuple_geometry_gpu.py.

The hard parts of the tuple path (pisces_hip_call_tiles / pisces_hip_accumulate_tiles / pisces_hip_add_observations) are geometry: where
a tile's segment starts relative to 16 bytes, how many batches it holds, which wave gets which of them, whether the last one is full,
where a log chunk ends, how far apart the tiles of one chunk are.  Here:

  * the batch sizes and chunk sizes, READ FROM THE SOURCE (csrc/kernels.hip.h, csrc/stream_kernels.hip.h): a kernel change that moves one
    moves the grid with it;
  * a model of each streaming loop as a function of (begin, end) that names the REGIME a segment puts the loop in (wave_model,
    block_model, ends_model), restated from the loops' control flow and from nothing else;
  * the grid: one tile per (start alignment, length) in two layouts (guards that are real observations / pad words), and a small second
    grid salted with tuples that must count for nothing;
  * two independent references: a numpy.bincount over the tuple fields, and the oracle's rows;
  * the observation-log cases (chunk edges, tiles further apart than the privatised range, drop and keep).

Exactness is the whole contract: every tuple counts once, nothing else counts.
"""
import os
import re
from types import SimpleNamespace

import numpy as np

from pisces_amd import _abi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pisces_amd", "csrc")
TILE = 64
MAX_BATCHES = 13         # the grid's longest segments; the regime enumeration runs over every segment up to this many batches
SEED = 20261019
GUARD_LOCUS = 5          # the guard words' locus field: an A of quality 37 on locus 5 of whichever tile reads it


# ------------------------------------------------------------------------------------------------------------------------------------
# constants from the source
# ------------------------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def parse_constants(kernels_text=None, stream_text=None):
    """PISCES_WAVE_UNROLL, kBlock, kUnroll, kGatherDirectTiles (kernels.hip.h), PISCES_LOG_CHUNK, kLocalTiles (stream_kernels.hip.h)."""
    kt = _source("kernels.hip.h") if kernels_text is None else kernels_text
    st = _source("stream_kernels.hip.h") if stream_text is None else stream_text

    def define(text, name):
        m = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert len(m) == 1, (name, m)
        return int(m[0])

    def constexpr(text, name):
        m = re.findall(r"\bconstexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(m) == 1, (name, m)
        return int(m[0])

    c = SimpleNamespace(wave_unroll=define(kt, "PISCES_WAVE_UNROLL"), block=constexpr(kt, "kBlock"), unroll=constexpr(kt, "kUnroll"),
                        gather_direct_tiles=constexpr(kt, "kGatherDirectTiles"), log_chunk=define(st, "PISCES_LOG_CHUNK"),
                        local_tiles=constexpr(st, "kLocalTiles"))
    # the constants the kernels derive from them must still be derived the same way
    assert re.search(r"constexpr\s+int\s+kWaveUnroll\s*=\s*PISCES_WAVE_UNROLL\s*;", kt)
    assert re.search(r"constexpr\s+uint32_t\s+kBatch\s*=\s*64u\s*\*\s*kWaveUnroll\s*;", kt)
    assert re.search(r"constexpr\s+int\s+kLogChunk\s*=\s*PISCES_LOG_CHUNK\s*;", st)
    c.wave_batch4 = 64 * c.wave_unroll          # dwordx4 of one wave batch (kBatch)
    c.B = 4 * c.wave_batch4                     # tuples of one wave batch
    c.block_iter4 = c.block * c.unroll          # dwordx4 of one iteration of the 256-thread form
    return c


K = parse_constants()


# ------------------------------------------------------------------------------------------------------------------------------------
# geometry models: (begin, end) -> regime
# ------------------------------------------------------------------------------------------------------------------------------------
def aligned_body(begin, end):
    """abegin, aend, degenerate as both loops compute them: the 16-byte-aligned body of tuples[begin, end)."""
    abegin, aend = (begin + 3) & ~3, end & ~3
    degenerate = abegin > aend          # no aligned dwordx4 AND the two roundings cross: the loops then fold everything into the head
    if degenerate:
        abegin = aend = end
    return abegin, aend, degenerate


def ends_model(begin, end):
    """The scalar loops around the body (the same in both forms): head words, tail words, the degenerate case, an empty body."""
    abegin, aend, degenerate = aligned_body(begin, end)
    return SimpleNamespace(head=abegin - begin, tail=end - aend, degenerate=degenerate, n4=(aend - abegin) >> 2)


def wave_model(begin, end, nw, k=K):
    """stream_tuples_wave<nw>: per wave (idle, pairs capped at 2, odd epilogue, last-batch mask applied), and whether the launch's last
    batch is exactly full."""
    e = ends_model(begin, end)
    n4, kb = e.n4, k.wave_batch4
    nb = (n4 + kb - 1) // kb
    waves = []
    for wid in range(nw):
        if not wid < nb:
            waves.append(SimpleNamespace(idle=True, pairs=0, odd=False, mask=False, batches=0))
            continue
        b = wid
        m = (nb - b + nw - 1) // nw
        pairs = (m - 1) // 2
        b += 2 * nw * pairs
        odd = ((m - 1) & 1) != 0
        if odd:
            b += nw
        mask = b == nb - 1 and n4 % kb != 0
        waves.append(SimpleNamespace(idle=False, pairs=min(pairs, 2), odd=odd, mask=mask, batches=m))
    assert sum(w.batches for w in waves) == nb
    return SimpleNamespace(ends=e, nb=nb, last_full=nb > 0 and n4 % kb == 0, waves=waves)


def block_model(begin, end, k=K):
    """stream_tuples (256 threads): iterations capped at 3, whether the last one is partial."""
    e = ends_model(begin, end)
    it = (e.n4 + k.block_iter4 - 1) // k.block_iter4
    return SimpleNamespace(ends=e, iterations=min(it, 3), partial=e.n4 % k.block_iter4 != 0)


def regimes_of(begin, end, k=K):
    """The names of every regime tuples[begin, end) puts a loop in.  A regime is one of
         ("ends", head, tail, degenerate, body empty)                     the scalar loops, shared by the forms
         ("wave1" | "wave2", wave, idle, pairs, odd, mask, last full)     one wave of a wave form
         ("block", iterations, partial)                                   the 256-thread form
    The scalar loops and the batch loop share abegin / aend and nothing else, so their regimes are counted side by side, not as a
    product."""
    e = ends_model(begin, end)
    out = [("ends", e.head, e.tail, e.degenerate, e.n4 == 0)]
    for nw in (1, 2):
        m = wave_model(begin, end, nw, k)
        for wid, w in enumerate(m.waves):
            out.append(("wave%d" % nw, wid, w.idle, w.pairs, w.odd, w.mask, m.last_full))
    b = block_model(begin, end, k)
    out.append(("block", b.iterations, b.partial))
    return out


def reachable_regimes(k=K, max_batches=MAX_BATCHES):
    """Every regime a segment of up to max_batches wave batches (plus its scalar ends) reaches, over the four alignments; the loop
    regimes depend on the body's dwordx4 count alone, so that is what is enumerated for them."""
    out = set()
    for a in range(4):
        for length in range(0, 12):
            out.update(regimes_of(a, a + length, k))
    for n4 in range(0, max_batches * k.wave_batch4 + 1):
        out.update(r for r in regimes_of(0, 4 * n4, k) if r[0] != "ends")
    for head in range(4):
        for tail in range(4):
            for n4 in (0, 1):
                begin = (4 - head) % 4
                out.add(regimes_of(begin, begin + head + 4 * n4 + tail, k)[0])
    return out


def describe(begin, end, k=K):
    return "; ".join(" ".join(str(x) for x in r) for r in regimes_of(begin, end, k))


# ------------------------------------------------------------------------------------------------------------------------------------
# the grid
# ------------------------------------------------------------------------------------------------------------------------------------
def grid_lengths(k=K, max_batches=MAX_BATCHES):
    """0..8 and k B + d, d in {-1, 0, +1, +3, +4}: with a batch of B tuples that is every loop regime.  None of those lengths is 2 modulo
    4 beyond 6, so a head of three words never met a tail of three around a body that is not empty: 9..11, B + 2 and 2 B + 2 add that."""
    return sorted(set(range(0, 12)) | {kk * k.B + d for kk in range(1, max_batches + 1) for d in (-1, 0, 1, 3, 4)} | {k.B + 2, 2 * k.B + 2})


def draw_tuples(rng, n, n_loci):
    """n observations of a tile of n_loci loci: (locus, tuple with that locus)."""
    locus = rng.integers(0, n_loci, n)
    allele = rng.choice(6, n, p=[.3, .2, .2, .2, .02, .08])
    qual = np.where(allele == 5, 255, rng.choice([5, 19, 20, 37], n))
    tup = _abi.tuple_pack(locus.astype(np.uint32), rng.integers(0, 11, n), rng.integers(0, 3, n), allele, qual)
    return locus.astype(np.int32), tup.astype(np.uint32)


def guard_word():
    return np.uint32(_abi.tuple_pack(GUARD_LOCUS, 5, 0, _abi.ALLELE_A, 37))


def lay_out(segments, alignments, n_loci, layout):
    """The tuple buffer and the PiscesTile array of `segments` (one uint32 array per tile, tile t on loci 64 t + 1 ..).
    layout "guarded": 1..7 guard words in front of every segment, so many that segment t starts at alignments[t] modulo 4, and 1..7 behind the
    last; nothing is padded.  layout "padded": every segment starts on a multiple of four and is filled up with PISCES_TUPLE_PAD, as
    bucket_scan_kernel lays segments out."""
    tiles = np.zeros(len(segments), dtype=_abi.TILE_DTYPE)
    parts, cursor = [], 0
    g = guard_word()
    for t, seg in enumerate(segments):
        if layout == "guarded":
            n_guard = (alignments[t] - cursor - 1) % 4 + 1        # 1..4
            if t % 3 == 2:
                n_guard += 4                                      # 5..8 -> keep it in 1..7
                if n_guard == 8:
                    n_guard = 4
            parts.append(np.full(n_guard, g, np.uint32))
            cursor += n_guard
            assert cursor % 4 == alignments[t] and 1 <= n_guard <= 7
        else:
            assert cursor % 4 == 0
        tiles[t] = (1 + TILE * t, n_loci[t], cursor, cursor + len(seg))
        parts.append(seg)
        cursor += len(seg)
        if layout == "padded":
            fill = -len(seg) % 4
            parts.append(np.full(fill, _abi.TUPLE_PAD, np.uint32))
            cursor += fill
    if layout == "guarded":
        parts.append(np.full(1 + len(segments) % 7, g, np.uint32))
    return np.concatenate(parts).astype(np.uint32), tiles


def make_reference(rng, n):
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    ref[rng.integers(0, n, max(1, n // 500))] = ord("N")
    return ref.astype(np.uint8)


def _finish(cells, segments, loci, n_loci, ref):
    pos = np.concatenate([1 + TILE * t + l for t, l in enumerate(loci)]).astype(np.int32) if segments else np.zeros(0, np.int32)
    tup = np.concatenate(segments).astype(np.uint32) if segments else np.zeros(0, np.uint32)
    g = SimpleNamespace(cells=cells, segments=segments, n_loci=np.asarray(n_loci, np.int32), n_tiles=len(segments), ref=ref,
                        region_loci=TILE * len(segments), positions=pos, tuples=tup)
    alignments = [a for a, _ in cells]
    g.layouts = {name: lay_out(segments, alignments, n_loci, name) for name in ("guarded", "padded")}
    return g


_CACHE = {}


def build_grid(k=K, seed=SEED):
    """One 64-locus tile per (alignment a in 0..3, length L in grid_lengths()), tile t on loci 64 t + 1 .. 64 t + 64."""
    key = ("grid", k.B, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        cells = [(a, length) for length in grid_lengths(k) for a in range(4)]
        segments, loci = [], []
        for _, length in cells:
            l, t = draw_tuples(rng, length, TILE)
            loci.append(l)
            segments.append(t)
        _CACHE[key] = _finish(cells, segments, loci, [TILE] * len(cells), make_reference(rng, TILE * len(cells) + 40))
    return _CACHE[key]


def cell_name(g, t, layout="guarded"):
    """What a failing assertion says about tile t: its (a, L) and its regimes from the models."""
    tile = g.layouts[layout][1][t]
    return "tile %d (a=%d, L=%d) [%s] %s" % (t, g.cells[t][0], g.cells[t][1], layout, describe(int(tile["tuple_begin"]), int(tile["tuple_end"])))


# the second, small grid: tuples that must count for nothing
INERT_TILE_LOCI = (64, 56, 7, 1)
INERT_KINDS = ("locus >= n_loci", "allele 6", "allele 7", "direction 3", "anchor 11..15", "pad word")


def inert_lengths(k=K):
    return (5, k.B - 1, k.B + 1)


def inert_tuple(rng, kind, n_loci):
    """One tuple of `kind` that is otherwise a plausible observation of the tile."""
    locus, anchor, direction, qual = int(rng.integers(0, n_loci)), int(rng.integers(0, 11)), int(rng.integers(0, 3)), 37
    allele = int(rng.integers(0, 4))
    if kind == "locus >= n_loci":
        if n_loci == TILE:
            return None                                    # six column bits cannot say 64
        locus = int(rng.integers(n_loci, TILE))
    elif kind == "allele 6":
        allele = 6
    elif kind == "allele 7":
        allele = 7
    elif kind == "direction 3":
        direction = 3
    elif kind == "anchor 11..15":
        anchor = int(rng.integers(11, 16))
    elif kind == "pad word":
        return np.uint32(_abi.TUPLE_PAD)
    else:
        raise ValueError(kind)
    return np.uint32(_abi.tuple_pack(locus, anchor, direction, allele, qual))


def build_inert_grid(k=K, seed=SEED + 1, kinds=INERT_KINDS):
    """Tiles of 64, 56, 7 and 1 loci x lengths {5, B-1, B+1} x alignments 0..3, plain and salted: salted.segments[t] is plain.segments[t]
    with inert tuples inserted at seeded places and, for the long ones, into the last aligned dwordx4 and the tail words (the salted
    segment keeps the plain one's start alignment; its length grows by the salt).  kinds: salt with these only (the plain grid is the
    same whatever they are).  Returns (plain, salted, kinds per tile)."""
    key = ("inert", k.B, seed, tuple(kinds))
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    cells, segs, loci, n_loci = [], [], [], []
    for nl in INERT_TILE_LOCI:
        for length in inert_lengths(k):
            for a in range(4):
                cells.append((a, length))
                l, t = draw_tuples(rng, length, nl)
                loci.append(l)
                segs.append(t)
                n_loci.append(nl)
    ref = make_reference(rng, TILE * len(cells) + 40)
    plain = _finish(cells, segs, loci, n_loci, ref)
    salted_segs, kinds_of = [], []
    for t, seg in enumerate(segs):
        words, salted_kinds = list(seg), []
        salt = [(kind, inert_tuple(rng, kind, n_loci[t])) for kind in kinds for _ in range(2)]
        salt = [(kind, w) for kind, w in salt if w is not None]
        for kind, w in salt:
            words.insert(int(rng.integers(0, len(words) + 1)), w)
            salted_kinds.append(kind)
        # the last word of the segment (a tail word or the last aligned dwordx4) and the one four in front of it, every kind in turn
        for j in range(2):
            at = len(words) if j == 0 else len(words) - 4
            w, turn = None, 2 * t + j
            while w is None and turn < 2 * t + j + len(kinds):     # (a 64-locus tile has no locus beyond it: the next kind)
                kind = kinds[turn % len(kinds)]
                w = inert_tuple(rng, kind, n_loci[t])
                turn += 1
            if w is not None:
                words.insert(max(at, 0), w)
                salted_kinds.append(kind)
        salted_segs.append(np.array(words, np.uint32))
        kinds_of.append(salted_kinds)
    salted = _finish([(a, len(s)) for (a, _), s in zip(cells, salted_segs)], salted_segs, loci, n_loci, ref)
    salted.positions, salted.tuples = plain.positions, plain.tuples      # what counts is the plain grid's
    _CACHE[key] = (plain, salted, kinds_of)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# the two references
# ------------------------------------------------------------------------------------------------------------------------------------
def count_tensor(positions, tuples, region_loci, min_bq=20, region_start=1):
    """int32[locus][6][3][11]: every tuple counted once under its fields, "allele < 4 and quality < minBQ gives N"."""
    _, anchor, direction, allele, qual = _abi.tuple_fields(np.asarray(tuples, np.uint32))
    allele = np.where((allele < 4) & (qual < min_bq), 4, allele).astype(np.int64)
    assert allele.max(initial=0) < 6 and direction.max(initial=0) < 3 and anchor.max(initial=0) < _abi.NUM_ANCHORS
    cell = ((np.asarray(positions, np.int64) - region_start) * 6 + allele) * 3 + direction.astype(np.int64)
    flat = np.bincount(cell * _abi.NUM_ANCHORS + anchor.astype(np.int64), minlength=region_loci * _abi.COUNTS_PER_LOCUS)
    assert flat.sum() == len(tuples)
    return flat.astype(np.int32).reshape(region_loci, 6, 3, _abi.NUM_ANCHORS)


def oracle_rows(g, cfg):
    from tests import orc
    key = ("rows", id(g), bytes(cfg))
    if key not in _CACHE:
        _CACHE[key] = orc.run_observations(g.positions, g.tuples, g.ref, 1, g.region_loci, cfg)
    return _CACHE[key]


def rows_agree_with_tensor(rows, tensor, ref, region_start=1):
    """The oracle's rows against the count tensor, folded over anchors as the oracle folds them (CoverageCalculator.CalculateSinglePoint):
    coverage by direction = A + C + G + T + deletion, no-calls = N, support by direction = the row's allele, reference support = the
    reference base's count.  Returns the number of cells compared."""
    folded = tensor.sum(axis=3, dtype=np.int64)                         # [locus][6][3]
    li = rows["position"].astype(np.int64) - region_start
    cov = folded[:, [0, 1, 2, 3, 5], :].sum(axis=1)                     # [locus][3]
    np.testing.assert_array_equal(rows["coverage_by_dir"], cov[li])
    np.testing.assert_array_equal(rows["total_coverage"], cov[li].sum(axis=1))
    np.testing.assert_array_equal(rows["num_no_calls"], folded[li, 4, :].sum(axis=1))
    info = rows["info"].astype(np.int64)
    alt, rt = _abi.info_alt(info), _abi.info_ref(info)
    real = alt < 6                                                      # (the Reference row over an N base is supported by the N count)
    assert real.all()
    np.testing.assert_array_equal(rows["support_by_dir"], folded[li, alt, :])
    np.testing.assert_array_equal(rows["allele_support"], folded[li, alt, :].sum(axis=1))
    known = rt < 4
    letters = np.frombuffer(_abi.BASE_OF_ALLELE.encode(), np.uint8)
    np.testing.assert_array_equal(letters[rt[known]], np.asarray(ref)[li[known] + region_start - 1])
    np.testing.assert_array_equal(rows["reference_support"][known], folded[li[known], rt[known], :].sum(axis=1))
    return int(len(rows) * 9 + real.sum() * 4 + known.sum())


def rows_by_tile(rows, n_tiles, region_start=1):
    return np.bincount((rows["position"].astype(np.int64) - region_start) // TILE, minlength=n_tiles)


# ------------------------------------------------------------------------------------------------------------------------------------
# the observation log (pisces_hip_add_observations): chunk edges, far tiles
# ------------------------------------------------------------------------------------------------------------------------------------
BLOCK = 1000                                     # GlobalConstants.RegionSize, the default block size
TILES_PER_BLOCK = (BLOCK + TILE - 1) // TILE


def log_tile_of(positions):
    """Tile index of a position in a bucketing of every block from the first on (bucket_tile_of on the regular grid: the block's first
    tile + offset / 64; a block of 1000 loci is 16 tiles)."""
    p = np.asarray(positions, np.int64) - 1
    return (p // BLOCK) * TILES_PER_BLOCK + (p % BLOCK) // TILE


def chunk_spans(positions, k=K):
    """Per log chunk of PISCES_LOG_CHUNK entries, in the order the entries were added: (lowest tile, highest tile, entries)."""
    t = log_tile_of(positions)
    return [(int(t[i:i + k.log_chunk].min()), int(t[i:i + k.log_chunk].max()), len(t[i:i + k.log_chunk])) for i in range(0, len(t), k.log_chunk)]


def observations(rng, positions):
    n = len(positions)
    allele = rng.choice(6, n, p=[.3, .2, .2, .2, .02, .08])
    qual = np.where(allele == 5, 255, rng.choice([5, 19, 20, 37], n))
    tup = _abi.tuple_pack(np.zeros(n, np.uint32), rng.integers(0, 11, n), rng.integers(0, 3, n), allele, qual)
    return np.asarray(positions, np.int32), tup.astype(np.uint32)


def chunk_edge_sizes(k=K):
    c = k.log_chunk
    return [c - 1, c, c + 1, 2 * c - 1, 2 * c + 1, 2 * c + 255, 2 * c + 257]


CHUNK_EDGE_LOCI = 3000


def chunk_edge_case(n, seed=SEED + 2):
    """n entries over 3000 loci (three blocks), positions shuffled: a chunk holds many tiles, a tile's entries come from many chunks.
    Added in three calls of unequal size (`parts`)."""
    rng = np.random.default_rng(seed + n)
    pos = np.concatenate([np.arange(1, CHUNK_EDGE_LOCI + 1), rng.integers(1, CHUNK_EDGE_LOCI + 1, n - CHUNK_EDGE_LOCI)]) if n >= CHUNK_EDGE_LOCI \
        else rng.integers(1, CHUNK_EDGE_LOCI + 1, n)
    rng.shuffle(pos)
    pos, tup = observations(rng, pos)
    cuts = [0, n // 7, n // 7 + n // 2 + 1, n]
    return SimpleNamespace(positions=pos, tuples=tup, parts=[slice(cuts[i], cuts[i + 1]) for i in range(3)], region_loci=CHUNK_EDGE_LOCI,
                           ref=make_reference(rng, CHUNK_EDGE_LOCI + 40))


FAR_LOCI = 70000


def far_tile_case(seed=SEED + 3):
    """70 000 loci (70 blocks, 1120 tiles) at depth 2 or 3.  The first layer of entries alternates between the lowest and the highest
    positions not yet used, so its first chunks hold entries of the first and of the last block: tiles kLocalTiles and more apart, the
    far ones counted and scattered one global atomic each.  The next layers run in position order: the same far tiles then get entries
    through the privatised branch of later chunks."""
    rng = np.random.default_rng(seed)
    asc = np.arange(1, FAR_LOCI + 1)
    zig = np.empty(FAR_LOCI, np.int64)
    zig[0::2] = asc[:FAR_LOCI // 2]
    zig[1::2] = asc[::-1][:FAR_LOCI // 2]
    third = np.sort(rng.choice(asc, FAR_LOCI // 2, replace=False))
    pos, tup = observations(rng, np.concatenate([zig, asc, third]))
    n = len(pos)
    cuts = [0, n // 5, n // 5 + n // 3 + 1, n]
    return SimpleNamespace(positions=pos, tuples=tup, parts=[slice(cuts[i], cuts[i + 1]) for i in range(3)], region_loci=FAR_LOCI,
                           ref=make_reference(rng, FAR_LOCI + 40), first_layer=FAR_LOCI)


def salted_observations(case, seed=SEED + 4, n_salt=400):
    """The case's entries with n_salt inert ones (allele codes 6 and 7, direction 3, anchors 11..15, pad words) shuffled in, on positions of
    the case: (positions, tuples).  What counts is the case's own entries."""
    rng = np.random.default_rng(seed)
    kinds = [k for k in INERT_KINDS if k != "locus >= n_loci"]
    tup = np.array([inert_tuple(rng, kinds[i % len(kinds)], TILE) for i in range(n_salt)], np.uint32)
    pos = rng.choice(case.positions, n_salt).astype(np.int32)
    order = rng.permutation(len(case.positions) + n_salt)
    return np.concatenate([case.positions, pos])[order], np.concatenate([case.tuples, tup])[order]
