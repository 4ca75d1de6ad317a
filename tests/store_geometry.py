"""The read store's flush at every fragment geometry: infrastructure of tests/test_store_geometry_cpu.py and
tests/test_store_geometry_gpu.py.

call_store_tiles_kernel (pisces_amd/csrc/store_kernels.hip.h) takes a flush from reads in HBM to called records; its inner walk,
walk_segment_fast, is geometry: one 16-byte fragment per CIGAR operation, (fragment, half-tile) pairs listed by two ballots, units of
sixteen pairs masked by an 81-entry table, blocks of 64 fragments dealt to 1..16 waves, the floor DoneProcessing leaves behind, a
fragment range from a position grid or a 32-ary search, a lane-per-locus pass for deletion fragments and a base-by-base fall-back.  Here:

  * the constants, READ FROM THE SOURCE (kernels.hip.h, store_kernels.hip.h, surface_store.inc.h): a kernel change that moves one moves
    the grid and its coverage proof with it;
  * a model of the kernel's CONTROL DECISIONS (never its counting) over reads, a flush schedule, a tile start and a wave count: which
    fragments shape_reads cuts a read into, which range of them a tile takes and how it is found, which pairs list_pairs lists, the
    composition of every block of 64, the mask-table entry and the load offset of every lane group, the floor's cut, the deletion
    pass and the general walk's blocks.  The model names the REGIME each of those is put in;
  * the grid: scenes of named cases, each case its own few tiles;
  * the required regimes, as data (REQUIRED), and the (empty) list of regimes deliberately left unreached (UNREACHED);
  * a numpy statement of RegionStateManager.AddAlleleCounts written from the reference's C# (RegionStateManager.cs:83-220,
    CandidateVariantFinder.cs:294-320), the second reference next to the oracle.

The model's segments are the batches ("every batch its own segment" of tests/test_read_store.py STORE_MODES) and, as a second reading,
all batches appended to one segment; the default mode takes one or the other by the batch's size.  Exactness is the whole contract:
every aligned base and every counted deleted position counts once, on its own locus and row, and nothing else counts.
"""
import bisect
import collections
import os
import re
from types import SimpleNamespace

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pisces_amd", "csrc")
SEED = 20261101
BLOCK = 1000                      # GlobalConstants.RegionSize, the default block size
WAVES = (1, 2, 4, 8, 16)
NUM_ANCHORS = 11                  # anchor size 5: bins 0..4 from the left end, 5 well anchored, 6..10 from the right end
ANCHOR_SIZE = 5
DIR_FORWARD, DIR_REVERSE, DIR_STITCHED = 0, 1, 2
ALLELE_OF = {ord("A"): 0, ord("G"): 1, ord("C"): 2, ord("T"): 3}     # AlleleType.cs: A, G, C, T, N, Deletion
ALLELE_N, ALLELE_DEL = 4, 5


# ------------------------------------------------------------------------------------------------------------------------------------
# constants from the source
# ------------------------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, head):
    """The text of the function whose head matches `head`, up to the next function at column 0."""
    m = re.search(head, text)
    assert m, head
    end = re.search(r"^}\s*$", text[m.end():], re.M)
    assert end, head
    return text[m.start():m.end() + end.end()]


def parse_constants(kernels_text=None, store_text=None, surface_text=None):
    """kTile (kernels.hip.h); kPairSlots, kSegmentPad, kGridGapCells, kDescLenMask, kMaskTab, kMaxSegments, the 16-bit span and delta fields,
    the block of 64 fragments, the unit of 16 pairs, the general walk's sub-chunk of 16 (store_kernels.hip.h); the wave-count rule of
    launch_call_store_tiles (surface_store.inc.h)."""
    kt = _source("kernels.hip.h") if kernels_text is None else kernels_text
    st = _source("store_kernels.hip.h") if store_text is None else store_text
    su = _source("surface_store.inc.h") if surface_text is None else surface_text

    def constexpr(text, name, ctype=r"int"):
        m = re.findall(r"\bconstexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), text)
        assert len(m) == 1, (name, m)
        expr = m[0].strip()
        assert re.fullmatch(r"[0-9a-fA-FxXu+*\s]+", expr), (name, expr)
        return int(eval(re.sub(r"(?<=[0-9a-fA-F])u\b", "", expr), {"__builtins__": {}}))

    c = SimpleNamespace(tile=constexpr(kt, "kTile"), pair_slots=constexpr(st, "kPairSlots"), segment_pad=constexpr(st, "kSegmentPad"),
                        grid_gap_cells=constexpr(st, "kGridGapCells"), desc_len_mask=constexpr(st, "kDescLenMask", "uint32_t"),
                        mask_tab=constexpr(st, "kMaskTab"), max_segments=constexpr(st, "kMaxSegments"),
                        delta_shift=constexpr(st, "kFragDeltaShift"), span_shift=constexpr(st, "kFragSpanShift"))
    c.delta_bits, c.span_bits = 64 - c.delta_shift, c.delta_shift - c.span_shift
    c.delta_max, c.span_max = (1 << c.delta_bits) - 1, (1 << c.span_bits) - 1
    # shape_reads states the two field limits itself: they must be the fields' widths
    shape = _body(st, r"__device__ __forceinline__ void shape_reads\(")
    m = re.findall(r"bool generic = ref_span > (0x[0-9A-Fa-f]+)ll \|\| gap_chain;", shape)
    assert len(m) == 1 and int(m[0], 16) == c.span_max, m
    m = re.findall(r"counted && first >= 0 && first <= (0x[0-9A-Fa-f]+)\)", shape)
    assert len(m) == 1 and int(m[0], 16) == c.delta_max, m
    assert re.search(r"frag_delta\(long long aoff\) \{ return \(int\)\(\(unsigned long long\)aoff >> %d\); \}" % c.delta_shift, st)
    fast = _body(st, r"__device__ __forceinline__ void walk_segment_fast\(")
    m = re.findall(r"const int n_blocks = \(hi - lo \+ (\d+)\) >> (\d+);", fast)
    assert len(m) == 1 and int(m[0][0]) == (1 << int(m[0][1])) - 1, m
    c.block = 1 << int(m[0][1])
    m = re.findall(r"const int ul = \(nl \+ (\d+)\) >> (\d+), ur = \(nr \+ (\d+)\) >> (\d+);", fast)
    assert len(m) == 1 and m[0][0] == m[0][2] and m[0][1] == m[0][3] and int(m[0][0]) == (1 << int(m[0][1])) - 1, m
    c.unit = 1 << int(m[0][1])
    m = re.findall(r"const bool left = pr < min\(er, (\d+)\), right = max\(pr, (\d+)\) < er;", fast)
    assert len(m) == 1 and m[0][0] == m[0][1], m
    c.half = int(m[0][0])
    assert c.half * 2 == c.tile and c.pair_slots == 2 * c.block + 2 * c.unit and c.mask_tab == 9 * 9
    c.lane_bytes = 8                                   # a lane's eight code bytes (load_u64_unaligned): the mask table is 9 x 9 for it
    assert re.search(r"const unsigned long long c8 = load_u64_unaligned\(codes \+ at\);", fast)
    general = _body(st, r"__device__ __forceinline__ void walk_segment\(")
    m = re.findall(r"const int src = (\d+) \* q \+ 4 \* u \+ g;", general)
    assert len(m) == 1, m
    c.sub_chunk = int(m[0])
    assert c.block % c.sub_chunk == 0 and re.search(r"min\(max\(s0, -3\), max\(len - 1, -3\)\)", general)
    # the wave-count rule
    launch = _body(su, r"static hipError_t launch_call_store_tiles\(")
    c.waves = tuple(sorted(int(x) for x in re.findall(r"PISCES_LAUNCH_STORE\((\d+)\);", launch)))
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", launch, flags=re.S))
    m = re.search(r"\(int64_t\)n_tiles <= \(int64_t\)h->n_cus \? (\d+) : \(int64_t\)n_tiles \* (\d+) <= \(int64_t\)h->n_cus \* (\d+) \? (\d+) : "
                  r"\(int64_t\)n_tiles <= \(int64_t\)h->n_cus \* (\d+) \? (\d+) : (\d+);", flat)
    assert m, "the wave-count rule of launch_call_store_tiles"
    c.wave_rule = tuple(int(x) for x in m.groups())
    return c


def waves_for(n_tiles, n_cus, k=None):
    """Waves a tile of a flush of n_tiles tiles, as launch_call_store_tiles picks them when PISCES_HIP_STORE_WAVES does not."""
    k = K if k is None else k
    w0, mul, cus_mul, w1, cus32, w2, w3 = k.wave_rule
    if n_tiles <= n_cus:
        return w0
    if n_tiles * mul <= n_cus * cus_mul:
        return w1
    return w2 if n_tiles <= n_cus * cus32 else w3


K = parse_constants()


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: control decisions, no counting
# ------------------------------------------------------------------------------------------------------------------------------------
REF_OPS, READ_OPS, ALIGNED_OPS = "MDN=X", "MIS=X", "M=X"


def ref_span_of(cigar):
    return sum(l for o, l in cigar if o in REF_OPS)


def shape_read(rd, min_bq=20, k=K):
    """shape_reads for one read: (read record, one fragment record per CIGAR operation)."""
    pos0, ops, q = rd["pos"], rd["cigar"], rd["quals"]
    n, nc = len(q), len(rd["cigar"])
    phase, lead, run, simple, prev_gap, gap_chain = 0, 0, 0, True, False, False
    for t, l in ops:
        if t in "DN":
            gap_chain, prev_gap = gap_chain or prev_gap, True
        if t in ALIGNED_OPS:
            prev_gap = False
            if phase == 2:
                simple = False
            phase, run = 1, run + l
        elif t == "S":
            if phase == 0:
                lead += l
            else:
                phase = 2
        elif t in "HP":
            if phase == 1 and t == "H":
                phase = 2
        else:
            simple = False
    ref_span = ref_span_of(ops)
    if run > k.desc_len_mask or run > n - lead:
        simple = False
    why = []
    if ref_span > k.span_max:
        why.append("span")
    if gap_chain:
        why.append("gap chain")
    if any(l > k.desc_len_mask for _, l in ops):
        why.append("operation length")
    generic = bool(why)
    read = SimpleNamespace(pos0=pos0, ref_span=ref_span, simple=simple, generic=generic, why=tuple(why), n=n, n_frags=nc)

    def dq(i):
        after = q[i]
        before = q[i - 1] if i > 0 else after
        return before >= min_bq and after >= min_bq

    ends_del = nc >= 1 and ops[-1][0] == "D"
    ends_del_soft = nc >= 2 and ops[-2][0] == "D" and ops[-1][0] == "S"
    frags, ri, rp, last_mapped = [], 0, pos0, pos0 - 1
    for c, (t, l) in enumerate(ops):
        f = SimpleNamespace(kind="empty", why="operation " + t, first=pos0, n=0, delta=rp - pos0, aoff=ri, counted=None, terminal=None, op=t)
        if generic:
            f.why = "generic"
        if t in "DN" and l > 0:
            idx, first, rj = -1, rp - pos0, ri
            for tk, lk in ops[c + 1:]:
                if idx >= 0:
                    break
                if tk in ALIGNED_OPS and lk > 0:
                    idx = rj
                elif tk in READ_OPS:
                    rj += lk
            counted = terminal = False
            if 0 <= idx < n:
                counted = dq(idx)
            elif t == "D" and c == nc - 1 and ends_del and n > 0:
                counted, first, terminal = dq(n - 1), last_mapped + 1 - pos0, True
            elif t == "D" and c == nc - 2 and ends_del_soft:
                at = n - ops[-1][1]
                if 0 <= at < n:
                    counted, first, terminal = dq(at), last_mapped + 1 - pos0, True
            f.counted, f.terminal, f.delta = counted, terminal, first
            if not generic:
                if counted and 0 <= first <= k.delta_max:
                    f.kind, f.why, f.first, f.n = "deletion", "", pos0 + first, l
                else:
                    f.why = "deletion not counted"
        elif t in ALIGNED_OPS and l > 0 and not generic:
            f.kind, f.why, f.first, f.n = "aligned", "", rp, max(min(l, n - ri), 0)
        frags.append(f)
        if t in REF_OPS:
            if t in READ_OPS and l > 0:
                last_mapped = rp + l - 1
            rp += l
        if t in READ_OPS:
            ri += l
    return read, frags


def shape_regimes(read, frags, k=K):
    """(a) of the model: the classes shape_reads puts a read's fragments in."""
    out = set()
    for f in frags:
        out.add(("shape", "kind", f.kind))
        out.add(("shape", "read", "generic: " + " + ".join(read.why) if read.generic else "simple" if read.simple else "complex"))
        half = 1 << (k.delta_bits - 1)
        if f.op in ALIGNED_OPS or f.op in "DN":
            out.add(("shape", "delta", "below 0x%X" % half if f.delta < half else "0x%X" % half if f.delta == half else "above 0x%X" % half))
            if f.delta == k.delta_max:
                out.add(("shape", "delta", "0x%X" % k.delta_max))
        if f.counted is not None:
            out.add(("shape", "deletion", "counted" if f.counted else "not counted", "terminal" if f.terminal else "closed by a base"))
    return out


def touched_blocks(rd, block=BLOCK):
    """Keys of the blocks a read can put a count in (aligned runs and gaps, whatever their quality: a superset only adds empty tiles)."""
    keys, rp = set(), rd["pos"]
    for t, l in rd["cigar"]:
        if t in REF_OPS and l > 0:
            keys.update(range((rp - 1) // block + 1, (rp + l - 2) // block + 2))
            rp += l
    return keys


class Segment:
    """The fragments of some batches as one segment of the store: arrays over fragments, in the order the reads were added."""

    def __init__(self, reads, min_bq=20, k=K):
        self.k, self.reads = k, reads
        pos0, first, n, kind, aoff, case, readi = [], [], [], [], [], [], []
        self.frags, self.shapes = [], set()
        base = 0
        for i, rd in enumerate(reads):
            read, frags = shape_read(rd, min_bq, k)
            self.shapes |= shape_regimes(read, frags, k)
            for f in frags:
                pos0.append(rd["pos"]); first.append(f.first); n.append(f.n)
                kind.append({"aligned": 0, "deletion": 1, "empty": 2}[f.kind]); aoff.append(base + f.aoff); readi.append(i)
                self.frags.append(f)
            base += len(rd["quals"])
        self.pos0, self.first, self.n = np.array(pos0, np.int64), np.array(first, np.int64), np.array(n, np.int64)
        self.kind, self.aoff, self.readi = np.array(kind, np.int64), np.array(aoff, np.int64), np.array(readi, np.int64)
        p = np.array([rd["pos"] for rd in reads], np.int64)
        self.sorted = bool((np.diff(p) >= 0).all())
        self.reach = max([min(ref_span_of(rd["cigar"]), 0x7FFFFFFF) for rd in reads] + [0])
        gaps = np.diff(p)
        self.grid_usable = self.sorted and not (gaps - 1 > k.grid_gap_cells).any()
        self.has_generic = any(f.why == "generic" for f in self.frags)
        self.n_floored_frags, self.floor = 0, 0
        self.last_end = max([rd["pos"] + ref_span_of(rd["cigar"]) - 1 for rd in reads] + [0])

    def search(self, x):
        """wave_lower_bound2's loop for one key: (answer, rounds, a probe fell inside a run of two or more fragments whose pos0 is x)."""
        a, b, rounds, tie, n = 0, len(self.pos0), 0, False, len(self.pos0)
        while b > a:
            rounds += 1
            step = max((b - a + 31) >> 5, 1)
            idx = a + (np.arange(32) + 1) * step - 1
            ok = idx < b
            v = self.pos0[np.minimum(idx, n - 1)]
            for i in idx[ok & (v == x)]:
                tie = tie or (i > 0 and self.pos0[i - 1] == x) or (i + 1 < n and self.pos0[i + 1] == x)
            c = int((ok & (v < x)).sum())
            na = a + c * step
            a, b = min(na, b), max(min(na + step - 1, b), min(na, b))
        return a, rounds, tie

    def range_of(self, tile_start):
        """(b) of the model: lo, hi, how they are found, the search's rounds and ties."""
        k = self.k
        x_lo, x_hi = max(tile_start - self.reach + 1, -0x7FFFFFFF), tile_start + k.tile
        if not self.sorted:
            return SimpleNamespace(lo=0, hi=len(self.pos0), method="scan", rounds=0, tie=False, x_lo=x_lo, x_hi=x_hi)
        lo, hi = bisect.bisect_left(self.pos0, x_lo), bisect.bisect_left(self.pos0, x_hi)
        if self.grid_usable:
            return SimpleNamespace(lo=lo, hi=hi, method="grid", rounds=0, tie=False, x_lo=x_lo, x_hi=x_hi)
        (a, r1, t1), (b, r2, t2) = self.search(x_lo), self.search(x_hi)
        assert (a, b) == (lo, hi), ((a, b), (lo, hi))
        return SimpleNamespace(lo=lo, hi=hi, method="search", rounds=max(r1, r2), tie=t1 or t2, x_lo=x_lo, x_hi=x_hi)


def tile_model(seg, tile_start, k=K):
    """(b)-(g) of the model for one segment and one tile: a namespace of per-fragment arrays over the tile's range, the blocks of 64 and
    the regimes (a set of tuples)."""
    T, H = k.tile, k.half
    r = seg.range_of(tile_start)
    sl = slice(r.lo, r.hi)
    idx = np.arange(r.lo, r.hi)
    kind, first, n0, pos0 = seg.kind[sl], seg.first[sl], seg.n[sl], seg.pos0[sl]
    floored = idx < seg.n_floored_frags
    floor_pos = np.where(floored, seg.floor, 0)
    n = np.where(kind == 0, n0, 0)
    pos = np.maximum(first, floor_pos)
    cut = np.minimum(pos - first, n)
    end = pos + (n - cut)
    pr, er = np.clip(pos - tile_start, 0, T), np.clip(end - tile_start, 0, T)
    left, right = pr < np.minimum(er, H), np.maximum(pr, H) < er
    reg = set()
    reg.add(("range", "method", r.method))
    if r.method == "search":
        reg.add(("range", "rounds", r.rounds))
        if r.tie:
            reg.add(("range", "tie run across a probe"))
    count = r.hi - r.lo
    reg.add(("range", "fragments", count))
    # (c) pairs
    cls = np.full(count, "", dtype=object)
    cls[left & ~right], cls[right & ~left], cls[left & right] = "left only", "right only", "both"
    none = ~left & ~right
    cls[none & (kind == 2)] = "none: an empty fragment"
    cls[none & (kind == 1)] = "none: a deletion fragment"
    al = none & (kind == 0)
    cls[al & (cut >= n) & (cut > 0)] = "none: below the floor"
    live = al & ~((cut >= n) & (cut > 0))
    cls[live & (end == tile_start)] = "none: ends on tile_start - 1"
    cls[live & (end < tile_start)] = "none: in range by reach only"
    cls[live & (pos >= tile_start + T)] = "none: begins behind the tile"
    cls[live & (n == 0) & (cls == "")] = "none: no base"
    assert (cls != "").all(), (tile_start, cls[cls == ""], pos[cls == ""], end[cls == ""])
    for c in set(cls.tolist()):
        reg.add(("pair", c))
    # (e) floor
    for fl, ct, nn, kd in set(zip(floored.tolist(), cut.tolist(), n.tolist(), kind.tolist())):
        if kd == 0:
            reg.add(("floor", "floored" if fl else "unfloored", "cut 0" if ct == 0 else "cut >= length" if ct >= nn else "cut positive"))
    # blocks of 64
    n_blocks = (count + k.block - 1) // k.block
    blocks = []
    for b in range(n_blocks):
        s = slice(b * k.block, min(count, (b + 1) * k.block))
        nl, nr = int(left[s].sum()), int(right[s].sum())
        blk = SimpleNamespace(nl=nl, nr=nr, ul=(nl + k.unit - 1) // k.unit, ur=(nr + k.unit - 1) // k.unit, count=s.stop - s.start,
                              mixed=bool(floored[s].any() and not floored[s].all()), dels=int((kind[s] == 1).sum()))
        blocks.append(blk)
        reg.add(("block", "pairs", nl, nr))
        reg.add(("block", "units", blk.ul, blk.ur))
        if blk.mixed:
            reg.add(("floor", "floored and unfloored in one block"))
    if n_blocks:
        reg.add(("block", "last block fragments", blocks[-1].count))
    for nw in k.waves:
        for w in range(nw):
            mine = max((n_blocks - w + nw - 1) // nw, 0)
            reg.add(("wave", nw, min(mine, 3)))
            if sum(1 for b in range(w, n_blocks, nw) if blocks[b].dels) > 1:
                reg.add(("deletion", "more than one block of a wave holds deletions"))
    # (d) units: per pair and lane group jj the mask-table entry and the load's place against the fragment's bytes
    for is_right, sel in ((0, left), (1, right)):
        if not sel.any():
            continue
        jj = np.arange(4)[None, :]
        rel = k.lane_bytes * jj + H * is_right                   # the lane's first locus
        a8 = np.clip(pr[sel][:, None] - rel, 0, k.lane_bytes)
        e8 = np.clip(er[sel][:, None] - rel, 0, k.lane_bytes)
        for a, e in set(zip(a8.ravel().tolist(), e8.ravel().tolist())):
            reg.add(("mask", a, e))
        p_un, e_un = (pos[sel] - tile_start)[:, None], (end[sel] - tile_start)[:, None]      # not clamped to the tile
        before = np.maximum(p_un - rel, 0)                       # bytes loaded in front of the first base still to count
        behind = np.maximum(rel + k.lane_bytes - e_un, 0)        # bytes loaded behind the last base
        assert before.max() < k.segment_pad and behind.max() < k.segment_pad
        reg.add(("load", "bytes before the fragment", int(before.max())))
        reg.add(("load", "bytes behind the fragment", int(behind.max())))
        resid = (seg.aoff[sl][sel][:, None] + cut[sel][:, None] + rel - p_un) % k.lane_bytes
        for x in set(resid.ravel().tolist()):
            reg.add(("load", "address mod 8", int(x)))
    # (f) the deletion pass
    d = kind == 1
    if d.any():
        df = np.maximum(np.maximum(first[d], floor_pos[d]), 1) - tile_start
        dl = first[d] + n0[d] - 1 - tile_start
        on = (df <= T - 1) & (dl >= 0) & (df <= dl)
        for a, b in set(zip(df[on].tolist(), dl[on].tolist())):
            if a == T - 1:
                reg.add(("deletion", "begins on locus 63"))
            if b == 0:
                reg.add(("deletion", "ends on locus 0"))
            if a <= 0 and b >= T - 1:
                reg.add(("deletion", "covers all 64 loci"))
            if a > 0 and b < T - 1:
                reg.add(("deletion", "inside the tile"))
        if (~on).any():
            reg.add(("deletion", "off the tile"))
    # (g) the general walk (GetCounts): blocks, sub-chunks, the load clamp
    reg.add(("general", "blocks", min(n_blocks, 3)))
    if n_blocks:
        reg.add(("general", "last block fragments mod 16", blocks[-1].count % k.sub_chunk))
        j4 = 4 * np.arange(T // 4)[None, :]
        s0 = tile_start + j4 - first[kind == 0][:, None]
        ln = n0[kind == 0][:, None]
        if s0.size:
            if (s0 < -3).any():
                reg.add(("general", "load clamp", "low end"))
            if (s0 > ln - 1).any():
                reg.add(("general", "load clamp", "high end"))
            if ((s0 >= -3) & (s0 <= ln - 1)).any():
                reg.add(("general", "load clamp", "none"))
    if seg.has_generic:
        reg.add(("generic", "the segment holds a generic read"))
    return SimpleNamespace(range=r, idx=idx, pr=pr, er=er, left=left, right=right, cls=cls, cut=cut, floored=floored, blocks=blocks, regimes=reg,
                           first=first, end=end, pos=pos, kind=kind, n0=n0)


def tile_starts(keys, tile_loci=None, block=BLOCK, k=K):
    """(tile start, loci) of every tile of the blocks `keys`, as regular_tile lays them out."""
    tl = k.tile if not tile_loci else tile_loci
    out = []
    for key in sorted(keys):
        b0 = (key - 1) * block + 1
        out += [(b0 + j, min(tl, block - j)) for j in range(0, block, tl)]
    return out


def flushes_of(scene, mode="own", min_bq=20, k=K):
    """The flushes of a scene's schedule: per flush the keys of the blocks it takes and the segments as they stand then.
    mode "own": every batch its own segment; "appended": one segment that every batch joins.  A flush up to position u takes the touched
    blocks whose last position is at most u (scenes keep candidate alleles from reaching across a flushed edge, the schedule's other
    condition); a segment none of whose reads reaches a block that is left goes (store_commit_flush)."""
    touched, done_key, out, segs, held = set(), 0, [], [], []
    schedule = list(zip(scene.batches, scene.ups)) + [([], None)]
    last = len(schedule) - 1
    for bi, (batch, up) in enumerate(schedule):
        if batch:
            held = held + list(batch)
            for rd in batch:
                touched |= touched_blocks(rd)
            if mode == "own":
                segs.append(Segment(list(batch), min_bq, k))
            else:
                old = segs[0] if segs else None
                g = Segment(held, min_bq, k)
                segs = [g if old is None else _refloored(g, old.n_floored_frags, old.floor)]
        if up is None and bi != last:
            continue
        keys = sorted(x for x in touched if x > done_key and (bi == last or x * BLOCK <= up))
        if not keys:
            continue
        out.append(SimpleNamespace(index=len(out), keys=keys, segments=list(segs), floors=[(g.n_floored_frags, g.floor) for g in segs]))
        done_key = keys[-1]
        floor = done_key * BLOCK + 1
        kept = []
        for g in segs:
            if g.last_end >= floor:
                kept.append(_refloored(g, len(g.pos0), max(g.floor, floor)))
            elif mode == "appended":
                held = []
        segs = kept
    return out


def _refloored(g, n_floored_frags, floor):
    """A view of segment g with another floor (the flush records of `flushes_of` keep the segment as it stood at their own flush)."""
    v = Segment.__new__(Segment)
    v.__dict__.update(g.__dict__)
    v.n_floored_frags, v.floor = n_floored_frags, floor
    return v


def case_of(scene, position):
    """The name of the case whose tiles hold `position`."""
    for name, lo, hi in scene.cases:
        if lo <= position <= hi:
            return name
    return "no case"


def scene_regimes(scene, mode="own", tile_loci=None, k=K):
    """{regime: set of (scene, case)} over every tile of every flush of the scene, and over the scene's fragments for (a)."""
    key = (scene.name, mode, tile_loci)
    if key in _CACHE:
        return _CACHE[key]
    out = collections.defaultdict(set)
    for fl in flushes_of(scene, mode, scene.min_bq, k):
        for g, (nf, floor) in zip(fl.segments, fl.floors):
            g = _refloored(g, nf, floor)
            if fl.index == 0:
                for rd in g.reads:
                    for reg in shape_regimes(*shape_read(rd, scene.min_bq, k), k):
                        out[reg].add((scene.name, rd.get("case", "no case")))
            for ts, _ in tile_starts(fl.keys, tile_loci, BLOCK, k):
                m = tile_model(g, ts, k)
                if len(m.idx):
                    who = (scene.name, g.reads[int(g.readi[m.idx[0]])].get("case", "no case"))
                else:
                    who = (scene.name, "empty tile " + case_of(scene, ts))
                for reg in m.regimes:
                    out[reg].add(who)
    _CACHE[key] = out
    return out


def describe_tile(scene, tile_start, mode="own", k=K):
    """What a failing assertion says about a tile: the case, the range and the block compositions of every segment at every flush that
    walks it, and the fragments that begin or end in it."""
    parts = ["case '%s', tile %d" % (case_of(scene, tile_start), tile_start)]
    for fl in flushes_of(scene, mode, scene.min_bq, k):
        if not any(ts == tile_start for ts, _ in tile_starts(fl.keys, None, BLOCK, k)):
            continue
        for si, (g, (nf, floor)) in enumerate(zip(fl.segments, fl.floors)):
            m = tile_model(_refloored(g, nf, floor), tile_start, k)
            if not len(m.idx):
                continue
            parts.append("flush %d segment %d: %s [%d, %d) floor %d (%d floored), blocks (nl, nr) %s" % (
                fl.index, si, m.range.method, m.range.lo, m.range.hi, floor, nf, " ".join("(%d,%d)" % (b.nl, b.nr) for b in m.blocks[:8])))
    return "; ".join(parts)


def describe_locus(scene, position, mode="own", k=K):
    """The tile of `position`, its regimes, and the fragments whose first or last position is `position`."""
    ts = (position - 1) // BLOCK * BLOCK + 1 + ((position - 1) % BLOCK) // k.tile * k.tile
    ends = []
    for rd in scene.reads:
        _, frags = shape_read(rd, scene.min_bq, k)
        for f in frags:
            if f.n and position in (f.first, f.first + f.n - 1):
                ends.append("%s %d+%d of read %d %s" % (f.kind, f.first, f.n, rd["pos"], cigar_string(rd["cigar"])))
    return "locus %d (%d of its tile): %s; fragments that begin or end here: %s" % (position, position - ts, describe_tile(scene, ts, mode, k),
                                                                                 ", ".join(ends[:6]) or "none")


def cigar_string(cigar):
    out, i = [], 0
    while i < len(cigar):
        j = i
        while j < len(cigar) and cigar[j] == cigar[i]:
            j += 1
        out.append("%d%s" % (cigar[i][1], cigar[i][0]) if j - i == 1 else "%dx(%d%s)" % (j - i, cigar[i][1], cigar[i][0]))
        i = j
    return "".join(out)


# ------------------------------------------------------------------------------------------------------------------------------------
# the required regimes (data) and the regimes deliberately left unreached
# ------------------------------------------------------------------------------------------------------------------------------------
COMPOSITIONS = [(0, 0), (1, 0), (0, 1), (15, 15), (16, 16), (17, 1), (1, 17), (32, 33), (48, 49), (63, 64), (64, 63), (64, 0), (0, 64), (64, 64)]
LAST_BLOCKS = [1, 15, 16, 17, 63, 64]
RANGES = [1, 64, 65, 128, 129]
PAIR_CLASSES = ["left only", "right only", "both", "none: in range by reach only", "none: ends on tile_start - 1", "none: an empty fragment",
                "none: a deletion fragment"]


def required_regimes(k=K):
    half = 1 << (k.delta_bits - 1)
    req = [("block", "pairs", nl, nr) for nl, nr in COMPOSITIONS]
    req += [("block", "last block fragments", n) for n in LAST_BLOCKS]
    req += [("range", "fragments", n) for n in RANGES]
    req += [("mask", a, e) for a in range(k.lane_bytes + 1) for e in range(k.lane_bytes + 1) if a < e]
    req += [("wave", nw, b) for nw in k.waves for b in range(4)]
    req += [("pair", c) for c in PAIR_CLASSES]
    # (a)
    req += [("shape", "kind", x) for x in ("aligned", "deletion", "empty")]
    req += [("shape", "read", x) for x in ("simple", "complex", "generic: span", "generic: gap chain")]
    req += [("shape", "delta", x) for x in ("below 0x%X" % half, "0x%X" % half, "above 0x%X" % half, "0x%X" % k.delta_max)]
    req += [("shape", "deletion", c, t) for c in ("counted", "not counted") for t in ("terminal", "closed by a base")]
    # (e)
    req += [("floor", "floored", c) for c in ("cut 0", "cut positive", "cut >= length")] + [("floor", "unfloored", "cut 0"),
                                                                                          ("floor", "floored and unfloored in one block")]
    # (f)
    req += [("deletion", x) for x in ("begins on locus 63", "ends on locus 0", "covers all 64 loci", "more than one block of a wave holds deletions")]
    # (b): every way a range is found, the search at one, two and three rounds, a tie run across a probe
    req += [("range", "method", x) for x in ("grid", "search", "scan")] + [("range", "rounds", x) for x in (1, 2, 3)] + [("range", "tie run across a probe")]
    # (g)
    req += [("general", "load clamp", x) for x in ("low end", "high end", "none")]
    return req


UNREACHED = []      # regimes of required_regimes() the grid deliberately does not reach: each entry needs a sentence in DESIGN section 5


# ------------------------------------------------------------------------------------------------------------------------------------
# the grid
# ------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


class Draw:
    """Seeded reads: bases i.i.d. A / C / G / T / N, qualities 5 / 19 / 20 / 37, the read's direction, and per-base directions where asked."""

    def __init__(self, seed, dirs=False):
        self.rng, self.dirs = np.random.default_rng(seed), dirs

    def read(self, pos, cigar, case, quals=None, dirs=None):
        if isinstance(cigar, str):
            from tests.orc import parse_cigar
            cigar = parse_cigar(cigar)
        rl = sum(l for o, l in cigar if o in READ_OPS)
        rd = {"pos": int(pos), "cigar": [(o, int(l)) for o, l in cigar], "case": case,
              "seq": bytes(self.rng.choice(np.frombuffer(b"ACGTN", np.uint8), rl, p=[.24, .24, .24, .24, .04]).astype(np.uint8)),
              "quals": (self.rng.choice([5, 19, 20, 37], rl, p=[.08, .08, .24, .6]).astype(np.uint8).tolist() if quals is None else list(quals)),
              "reverse": bool(self.rng.integers(0, 2))}
        assert len(rd["quals"]) == rl and pos >= 1
        if self.dirs or dirs is not None:
            rd["dirs"] = self.rng.integers(0, 3, rl).astype(np.uint8).tolist() if dirs is None else list(dirs)
        return rd


def tile_at(key, j, k=K):
    """First position of tile j of block `key` (64-locus tiles)."""
    return (key - 1) * BLOCK + 1 + k.tile * j


def make_reference(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)


def _scene(name, batches, ups, cases, seed, min_bq=20):
    reads = [rd for b in batches for rd in b]
    top = max(rd["pos"] + max(ref_span_of(rd["cigar"]), 1) for rd in reads)
    n_loci = ((top + 200) // BLOCK + 1) * BLOCK
    rng = np.random.default_rng(seed + 77)
    # where GetCounts looks: the blocks any read touches, merged into runs
    keys = sorted(set().union(*[touched_blocks(rd) for rd in reads]))
    return SimpleNamespace(name=name, batches=batches, ups=list(ups) + [None] * (len(batches) - len(ups)), cases=cases, reads=reads,
                           n_loci=n_loci, ref=make_reference(rng, n_loci + 40), min_bq=min_bq, keys=keys)


def _case_span(cases, name, key_lo, key_hi=None):
    cases.append((name, (key_lo - 1) * BLOCK + 1, (key_lo if key_hi is None else key_hi) * BLOCK))


# ---- exhaustive edges ---------------------------------------------------------------------------------------------------------------
EDGE_TILES = (("tile at position 1", 1, 0), ("tile inside a block", 3, 5), ("a block's last, short tile", 5, 15))
BEFORE, PAST = (1, 7, 8, 9, 63, 64, 65), (1, 7, 8, 9, 64)


def edge_reads(d, s, case, k=K):
    """Every (pr, er), 0 <= pr < er <= 64, as one single-M read on the tile at s, and the variants around its ends."""
    T, out = k.tile, []
    for pr in range(T):
        for er in range(pr + 1, T + 1):
            out.append(d.read(s + pr, [("M", er - pr)], case))
    for b in BEFORE:                       # pr = 0, begun b positions before the tile
        if s - b >= 1:
            for er in (1, k.half, k.half + 1, T):
                out.append(d.read(s - b, [("M", b + er)], case))
    for p in PAST:                         # er = 64, run p positions past it
        for pr in (0, k.half - 1, k.half, T - 1):
            out.append(d.read(s + pr, [("M", T - pr + p)], case))
    if s > 12:
        out.append(d.read(s - 10, [("M", 10)], case))       # ends on tile_start - 1
        out.append(d.read(s - 10, [("M", 11)], case))       # ends on tile_start
    out.append(d.read(s + T - 1, [("M", 5)], case))         # begins on tile_end
    out.append(d.read(s + T, [("M", 5)], case))             # begins on tile_end + 1
    return out


def edges_scene(dirs, seed):
    d, reads, cases = Draw(seed, dirs), [], []
    for name, key, j in EDGE_TILES:
        reads += edge_reads(d, tile_at(key, j), name)
        _case_span(cases, name, key, key + 1)
    reads.sort(key=lambda r: r["pos"])
    return _scene("edges, per-base directions" if dirs else "edges", [reads], [], cases, seed)


# ---- block composition --------------------------------------------------------------------------------------------------------------
def composition_kinds(nl, nr, block=64):
    """Kinds of one block of fragments with nl left and nr right pairs: L left only, R right only, B both, E empty; L and B before R (the
    reads are in position order), the empty ones in front of a block that begins with the right half and behind every other."""
    both = min(nl, nr)
    ls, rs = nl - both, nr - both
    fill = block - both - ls - rs
    assert fill >= 0
    body = ["L"] * ls + ["B"] * both + ["R"] * rs
    return ["E"] * fill + body if (nl <= 1 and nr >= 1) or not body else body + ["E"] * fill


def kinds_reads(d, s, kinds, case, k=K):
    """Reads on the tile at s whose fragments, in order, have the kinds given.  Empty fragments are H / P operations (and a soft clip)
    in front of the next read's aligned run, or behind the last read's."""
    H, T = k.half, k.tile
    n_left = sum(1 for x in kinds if x in "LB")
    n_right = sum(1 for x in kinds if x == "R")
    out, pending, il, ir = [], 0, 0, 0
    for x in kinds:
        if x == "E":
            pending += 1
            continue
        lead = [("HP"[i & 1], 1) for i in range(pending)]
        if pending and d.rng.integers(0, 3) == 0:
            lead[-1] = ("S", 2)
        pending = 0
        if x in "LB":
            off = (il * (H - 1)) // max(n_left, 1)
            il += 1
            ln = int(d.rng.integers(1, H - off + 1)) if x == "L" else H + 1 - off + int(d.rng.integers(0, 40))
        else:
            off = H + (ir * (H - 1)) // max(n_right, 1)
            ir += 1
            ln = int(d.rng.integers(1, T - off + 20))
        out.append(d.read(s + off, lead + [("M", ln)], case))
    if pending:
        assert out, "a run of empty fragments needs a read to hang on"
        last = out.pop()
        out.append(d.read(last["pos"], last["cigar"] + [("HP"[i & 1], 1) for i in range(pending)], case))
    return out


PILE = 3100            # fragments on one tile: 49 blocks, so that each of 16 waves has three or more


def blocks_scene(dirs, seed, k=K):
    d, reads, cases, key = Draw(seed, dirs), [], [], 2
    for nl, nr in COMPOSITIONS:
        name = "composition (%d, %d)" % (nl, nr)
        kinds = composition_kinds(nl, nr, k.block)
        if (nl, nr) == (0, 0):
            kinds = kinds + ["B"]                      # (the sixty-four empty fragments hang in front of a read of the next block)
        reads += kinds_reads(d, tile_at(key, 3), kinds, name)
        _case_span(cases, name, key)
        key += 1
    for n in sorted(set(RANGES + LAST_BLOCKS)):
        name = "range of %d fragments" % n
        reads += kinds_reads(d, tile_at(key, 7), ["B"] * n, name)
        _case_span(cases, name, key)
        key += 1
    # empty fragments (I, S, H, P) and reads in range by reach only, interleaved
    name, s = "empty fragments and reads in range by reach only", tile_at(key, 2)
    for i in range(40):
        reads.append(d.read(s - 60 + i, [("S", 1), ("M", 3), ("I", 2), ("M", 4), ("P", 1), ("M", 2), ("H", 1)], name))      # ends before the tile
        reads.append(d.read(s - 60 + i, [("M", 60 - i)], name))                                                              # ends on tile_start - 1
    for i in range(40):
        reads.append(d.read(s + i, [("H", 2), ("S", 3), ("M", 5), ("I", 1), ("M", 5 + i), ("P", 2), ("M", 3), ("S", 2)], name))
    _case_span(cases, name, key)
    key += 1
    name, s = "a pile of %d fragments on one tile" % PILE, tile_at(key, 4)
    for i in range(PILE):
        off = (i * k.tile) // PILE
        reads.append(d.read(s + off, [("M", int(d.rng.integers(1, 24)))], name))
    _case_span(cases, name, key)
    reads.sort(key=lambda r: r["pos"])
    return _scene("blocks, per-base directions" if dirs else "blocks", [reads], [], cases, seed)


# ---- reach and the fragment range ---------------------------------------------------------------------------------------------------
REACH = 200
FAR = 70_000


def reach_reads(d, key, tag):
    """The segment's longest read (span REACH) ending on a tile's first locus, ending one earlier on another tile, and a read one position
    before each range's start."""
    out, cases = [], []
    s = tile_at(key, 6)
    name = "longest read ends on tile_start" + tag
    out.append(d.read(s - REACH + 1, [("M", REACH)], name))             # pos0 == x_lo: the range's first fragment, counted once on locus 0
    out.append(d.read(s - REACH, [("M", 50)], name))                    # one position before the range's start
    out += [d.read(s + 3 * i, [("M", 30)], name) for i in range(10)]
    _case_span(cases, name, key)
    s = tile_at(key + 1, 6)
    name = "longest read ends on tile_start - 1" + tag
    out.append(d.read(s - REACH, [("M", REACH)], name))                 # pos0 == x_lo - 1: not in the range, and it does not reach
    out.append(d.read(s - REACH + 1, [("M", REACH - 1)], name))         # the range's first fragment, ends on tile_start - 1
    out += [d.read(s + 3 * i, [("M", 30)], name) for i in range(10)]
    _case_span(cases, name, key + 1)
    return out, cases


def reach_scene(seed):
    """One batch with the position grid, one (a far read behind a gap wider than kGridGapCells) without, one unsorted."""
    d = Draw(seed)
    grid, c1 = reach_reads(d, 2, ", grid")
    search, c2 = reach_reads(d, 5, ", search")
    search.append(d.read(FAR + 5 * BLOCK, [("M", 40)], "far read"))
    scan, c3 = reach_reads(d, 8, ", unsorted")
    grid.sort(key=lambda r: r["pos"])
    search.sort(key=lambda r: r["pos"])
    d.rng.shuffle(scan)
    assert any(a["pos"] > b["pos"] for a, b in zip(scan, scan[1:]))
    cases = c1 + c2 + c3
    _case_span(cases, "far read", FAR // BLOCK + 6)
    return _scene("reach", [grid, search, scan], [], cases, seed)


SEGMENT_SIZES = (1, 31, 32, 33, 1024, 1025, 1057)      # (32 probes a round: up to 32 fragments one round, up to 32 * 33 two, beyond three)


def search_scene(seed, k=K):
    """Segments of 1, 31, 32, 33, 1024, 1025 and 1057 fragments, each (but the one of one fragment) with its last read behind a gap wider than
    kGridGapCells, so that the 32-ary search finds the ranges: one, two and three rounds.  Then a segment whose search probes fall into a
    run of a hundred fragments with one pos0, which is x_lo of a tile."""
    d, batches, cases, key = Draw(seed), [], [], 2
    for n in SEGMENT_SIZES:
        name, s = "segment of %d fragments" % n, tile_at(key, 9)
        near = n - 1 if n > 1 else 1
        reads = [d.read(s - 20 + (i * 100) // near, [("M", int(d.rng.integers(5, 40)))], name) for i in range(near)]
        if n > 1:
            reads.append(d.read(FAR + key * BLOCK + 17, [("M", 33)], name))
        batches.append(reads)
        _case_span(cases, name, key)
        key += 1
    name, s = "a hundred fragments share the pos0 a probe lands in", tile_at(key, 9)
    pile_pos = s - REACH + 1
    reads = [d.read(pile_pos - 40 + i, [("M", 20)], name) for i in range(40)]
    reads += [d.read(pile_pos, [("M", REACH if i == 0 else int(d.rng.integers(10, 60)))], name) for i in range(100)]
    reads += [d.read(pile_pos + 1 + (i * (REACH + 80)) // 960, [("M", int(d.rng.integers(5, 50)))], name) for i in range(960)]
    reads.append(d.read(FAR + key * BLOCK + 17, [("M", 33)], name))
    batches.append(reads)
    _case_span(cases, name, key)
    _case_span(cases, "far reads", FAR // BLOCK + 2, FAR // BLOCK + key + 1)
    return _scene("search", batches, [], cases, seed)


# ---- the floor ----------------------------------------------------------------------------------------------------------------------
def floor_scene(n_flushes, seed, k=K):
    """SmallVariantCaller's schedule: the batch of block b is added, the blocks up to b are flushed, the next batch lands on block b + 1's
    first tiles.  The first batch's reads straddle the edge at every cut from 1 to 200 and stay in the store, floored; with every batch
    appended to one segment they share blocks of 64 with the next batch's reads.  Single-M reads and two-run reads (a pad operation between
    the runs: the second run begins behind the edge, cut 0) across the edge: an insertion or deletion candidate next to the edge would
    hold the block back (GetCandidatesToProcess keeps a block whose alleles reach past upTo), and the floor would never be laid.
    tests/test_store_geometry_gpu.py shows from GetCounts that every flush of the schedule takes its block."""
    d, batches, ups, cases = Draw(seed), [], [], []
    for b in range(n_flushes):
        key = 2 + b
        edge = key * BLOCK                                  # the block's last position; the floor after its flush is edge + 1
        name = "flush %d" % (b + 1)
        reads = []
        if b > 0:                                           # on this block's first tiles: unfloored, next to the floored straddlers
            reads += [d.read(edge - BLOCK + 1 + (i * 150) // 90, [("M", int(d.rng.integers(4, 70)))], name) for i in range(90)]
        reads += [d.read(edge - 400 + 2 * i, [("M", int(d.rng.integers(20, 120)))], name) for i in range(60 + 7 * b)]     # end below the edge: cut >= length
        reads += [d.read(edge + 1 - cut, [("M", 250 if cut % 3 else cut + int(d.rng.integers(1, 64)))], name) for cut in range(200, 0, -1)]
        # (the second run begins on edge + 2 - i: behind the floor, on it, and below it)
        reads += [d.read(edge - 18 - i, [("M", 20), ("P", 1), ("M", 31 + i + int(d.rng.integers(1, 50)))], name) for i in range(9)]
        reads += [d.read(edge - 10 - i, [("M", 5), ("I", 1), ("M", 4), ("S", 2)], name) for i in range(5)]               # both runs below the edge
        reads.sort(key=lambda r: r["pos"])
        batches.append(reads)
        ups.append(edge)
        _case_span(cases, name, key, key)
    key = 2 + n_flushes
    name = "after the last flush"
    reads = [d.read(key * BLOCK - BLOCK + 1 + (i * 150) // 90, [("M", int(d.rng.integers(4, 70)))], name) for i in range(90)]
    reads.sort(key=lambda r: r["pos"])
    batches.append(reads)
    ups.append(None)
    _case_span(cases, name, key, key + 1)
    return _scene("floor, %d flushes in a row" % n_flushes, batches, ups, cases, seed)


def late_scene(seed=SEED + 20, k=K):
    """Reads added after a flush that begin in the flushed block (the library accepts them, as RegionStateManager does: GetBlock makes the
    block anew).  Block 2 is flushed with reads across its edge left in the store, floored; then a batch arrives whose first reads begin
    below the floor, on the flushed block's last tiles.  At the final flush those tiles are walked again: the floored reads must not
    count there a second time, the late reads must count in full — the late batch's first fragment, whose index is n_floored_frags when
    the batch is appended to the segment, included.  The oracle's schedule entry adds every read before the first flush, so it cannot
    say this; the reference is DoneProcessing itself (late_tensor below; the CPU test drives orc.State through the same steps)."""
    d = Draw(seed)
    edge = 2 * BLOCK
    first = [d.read(edge - 300 + 2 * i, [("M", int(d.rng.integers(20, 90)))], "before the flush") for i in range(70)]
    first += [d.read(edge + 1 - cut, [("M", 150)], "before the flush") for cut in range(120, 0, -3)]
    first.sort(key=lambda r: r["pos"])
    late = [d.read(edge - 100 + i, [("M", 60 + 2 * i)], "late reads") for i in range(101)]       # begin below the floor; the last one begins on the edge
    late += [d.read(edge + 1 + 3 * i, [("M", int(d.rng.integers(10, 80)))], "late reads") for i in range(40)]
    late.sort(key=lambda r: r["pos"])
    assert len(first) % k.block != 0 and late[0]["pos"] + 60 <= edge       # (the first late fragment lies wholly below the floor)
    cases = [("before the flush", BLOCK + 1, edge), ("late reads", edge + 1, 3 * BLOCK)]
    return _scene("late reads", [first, late], [edge, None], cases, seed)


def late_tensor(scene, n_loci):
    """What the state holds once the late batch is in: DoneProcessing (RegionStateManager.cs:336-353) dropped the flushed blocks, so below
    the floor only the late reads count; from the floor on, every read."""
    floor = scene.ups[0] + 1
    out = count_tensor(scene.batches[1], 1, n_loci, scene.min_bq)
    out[floor - 1:] += count_tensor(scene.batches[0], 1, n_loci, scene.min_bq)[floor - 1:]
    return out


# ---- the 16-bit fields --------------------------------------------------------------------------------------------------------------
def fields_scene(op, seed, k=K):
    """Reference spans of 0xFFFE, 0xFFFF, 0x10000 and 0x10001 by a skip (op N) or by a deletion (op D), with a last run of 30 bases and of
    one (delta = span - 1); a second run exactly 0x8000 behind the read's position.  The deletions' own positions are counted on every
    tile up to the far end.  (The oracle's candidate records hold alleles of up to ORC_MAX_ALLELE bases, so the scene by D has no oracle
    rows: its flush is judged by the count tensor, ORACLE_ROWS below.)"""
    d, reads, cases = Draw(seed), [], []
    i = 0
    for op in op:
        for span in (k.span_max - 1, k.span_max, k.span_max + 1, k.span_max + 2):
            for tail in (30, 1):
                name = "span 0x%X by %s, last run %dM" % (span, op, tail)
                q = [37] * (20 + tail)
                reads.append(d.read(100 + 7 * i, [("M", 20), (op, span - 20 - tail), ("M", tail)], name, quals=q))
                i += 1
        half = 1 << (k.delta_bits - 1)
        for delta in (half - 1, half, half + 1):
            name = "second run 0x%X behind the read's position, by %s" % (delta, op)
            reads.append(d.read(100 + 7 * i, [("M", 20), (op, delta - 20), ("M", 25)], name, quals=[37] * 45))
            i += 1
    reads.sort(key=lambda r: r["pos"])
    cases.append(("the reads' first runs", 1, BLOCK))
    cases.append(("the gaps", BLOCK + 1, 32 * BLOCK))
    cases.append(("the runs 0x8000 behind", 32 * BLOCK + 1, 34 * BLOCK))
    cases.append(("the gaps, far half", 34 * BLOCK + 1, 65 * BLOCK))
    cases.append(("the far ends", 65 * BLOCK + 1, 67 * BLOCK))
    return _scene("fields by " + op, [reads], [], cases, seed)


# ---- deletions ----------------------------------------------------------------------------------------------------------------------
def deletions_scene(dirs, seed, k=K):
    d, reads, cases, key = Draw(seed, dirs), [], [], 2
    T = k.tile
    good = lambda n: [37] * n

    def add(name, j, make):
        nonlocal key
        s = tile_at(key, j)
        reads.extend(make(s, name))
        _case_span(cases, name, key)
        key += 1

    add("a deletion begins on locus 63", 4, lambda s, nm: [d.read(s + T - 1 - 10, [("M", 10), ("D", 3), ("M", 10)], nm, quals=good(20)) for _ in range(3)])
    add("a deletion ends on locus 0", 4, lambda s, nm: [d.read(s - 3 - 10 + 1, [("M", 10), ("D", 3), ("M", 10)], nm, quals=good(20)) for _ in range(3)])
    add("a deletion over a whole tile and its neighbours", 4,
        lambda s, nm: [d.read(s - 70 - 10, [("M", 10), ("D", 200), ("M", 10)], nm, quals=good(20)) for _ in range(3)] +
                      [d.read(s - 10, [("M", 10), ("D", T), ("M", 10)], nm, quals=good(20))] +
                      [d.read(s - 10, [("M", 10), ("N", T + 1), ("M", 10)], nm, quals=good(20))])
    low_close = good(10) + [5] + good(9)
    low_before = good(9) + [19] + good(10)
    add("a deletion closed by a low-quality base", 2, lambda s, nm: [d.read(s + 5 + i, [("M", 10), ("D", 4), ("M", 10)], nm, quals=low_close) for i in range(4)])
    add("the base before the closing base is low", 2, lambda s, nm: [d.read(s + 5 + i, [("M", 10), ("D", 4), ("M", 10)], nm, quals=low_before) for i in range(4)])
    add("10M3D2I10M: the closing base lies behind the insertion", 2,
        lambda s, nm: [d.read(s + 5 + i, "10M3D2I10M", nm, quals=q) for i, q in enumerate((good(22), good(11) + [5] + good(10), good(12) + [5] + good(9),
                                                                                           good(10) + [5] + good(11)))])
    add("terminal deletions", 2,
        lambda s, nm: [d.read(s + 5 + i, "12M3D", nm, quals=q) for i, q in enumerate((good(12), good(11) + [5], good(10) + [5, 37]))] +
                      [d.read(s + 30 + i, "12M3D2S", nm, quals=q) for i, q in enumerate((good(14), good(12) + [5, 37], good(11) + [5, 37, 37],
                                                                                       good(12) + [37, 5]))] +
                      [d.read(s + T - 13, "12M3D", nm, quals=good(12)), d.read(s - 14, "12M3D", nm, quals=good(12))])
    add("a deletion in front of the read's first base", 2, lambda s, nm: [d.read(s + 7, "3D10M", nm, quals=good(10)), d.read(s + 9, "2N10M", nm, quals=[5] + good(9))])
    add("gap chains against fragments", 2,
        lambda s, nm: [d.read(s + 3, "10M2D3N10M", nm, quals=good(20)), d.read(s + 4, "10M2D2I3D10M", nm, quals=good(22)),
                       d.read(s + 5, "10M2D1M3D10M", nm, quals=good(21)), d.read(s + 6, "10M2D3N10M", nm), d.read(s + 7, "10M2D1M3D10M", nm)])
    add("more than 128 deletion fragments in one tile's range", 5,
        lambda s, nm: [d.read(s - 8 + (i * 70) // 190, [("M", 6), ("D", 1 + i % 5), ("M", 6)], nm, quals=good(12) if i % 4 else None) for i in range(190)])
    reads.sort(key=lambda r: r["pos"])
    return _scene("deletions, per-base directions" if dirs else "deletions", [reads], [], cases, seed)


# ---- segments -----------------------------------------------------------------------------------------------------------------------
def batches_scene(seed, k=K):
    """Nine batches (more than the store has segments): one tile fed from two of them, one from seven, one from all nine.  Every batch is
    in position order; appended to one segment they are not."""
    d, cases = Draw(seed), []
    tiles = {2: tile_at(2, 3), 7: tile_at(4, 3), 9: tile_at(6, 3)}
    batches = []
    for b in range(9):
        reads = []
        for n_fed, s in tiles.items():
            if b < n_fed:
                reads += [d.read(s - 20 + int(d.rng.integers(0, 90)), [("M", int(d.rng.integers(5, 60)))], "a tile fed from %d batches" % n_fed) for _ in range(12)]
        reads.sort(key=lambda r: r["pos"])
        batches.append(reads)
    for n_fed, s in tiles.items():
        _case_span(cases, "a tile fed from %d batches" % n_fed, (s - 1) // BLOCK + 1)
    return _scene("batches", batches, [], cases, seed)


def ends_scene(pr_first, dirs, seed, k=K):
    """The first read of the segment's arrays begins on locus pr_first of its tile (nothing in front of it: the bytes before the arrays'
    first are loaded and masked), the last read of the arrays ends on locus 0 of its tile (er = 1: the bytes behind the arrays' last)."""
    d, cases = Draw(seed, dirs), []
    s0, s1 = tile_at(2, 3), tile_at(2, 9)
    name = "first read with pr = %d, last read with er = 1" % pr_first
    reads = [d.read(s0 + pr_first, [("M", 9)], name)] + [d.read(s0 + pr_first + 1 + 4 * i, [("M", 7 + i)], name) for i in range(5)]
    reads += [d.read(s1 - 30 + 3 * i, [("M", 6)], name) for i in range(6)] + [d.read(s1 - 9, [("M", 10)], name)]
    assert reads == sorted(reads, key=lambda r: r["pos"]) and reads[-1]["pos"] + 9 == s1
    _case_span(cases, name, 2)
    return _scene("ends of the arrays, pr = %d%s" % (pr_first, ", per-base directions" if dirs else ""), [reads], [], cases, seed)


def build_scenes(k=K, seed=SEED):
    key = ("scenes", seed)
    if key not in _CACHE:
        _CACHE[key] = [edges_scene(False, seed + 1), edges_scene(True, seed + 2), blocks_scene(False, seed + 3), blocks_scene(True, seed + 4),
                       reach_scene(seed + 5), search_scene(seed + 6), floor_scene(2, seed + 7), floor_scene(3, seed + 8), fields_scene("N", seed + 9), fields_scene("D", seed + 17),
                       deletions_scene(False, seed + 10), deletions_scene(True, seed + 11), batches_scene(seed + 12),
                       ends_scene(31, False, seed + 13), ends_scene(63, False, seed + 14), ends_scene(31, True, seed + 15), ends_scene(63, True, seed + 16)]
    return _CACHE[key]


def scene_named(name):
    return next(s for s in build_scenes() if s.name == name)


def read_batch(reads):
    from pisces_amd import _abi
    return _abi.ReadBatch([dict(rd) for rd in reads])


# ------------------------------------------------------------------------------------------------------------------------------------
# the two references
# ------------------------------------------------------------------------------------------------------------------------------------
def count_tensor(reads, region_start, region_loci, min_bq=20):
    """RegionStateManager.AddAlleleCounts (RegionStateManager.cs:118-220) over `reads` into int32[locus][6][3][11], from the reference's
    C#: the position map of the CIGAR, AlleleHelper.GetAlleleType with "quality below minBQ is an N" (:179-181), the direction of the
    base, GetAnchorType (:83-116); a gap's positions as deletions in the direction and anchor bin of the base that closes it if
    CandidateVariantFinder.CheckDeletionQuality passes there (:170-176), a deletion at the read's end or before its final soft clip in
    the last bin (:143-154, :195-210)."""
    P, A, D, AN = [], [], [], []       # positions, alleles, directions, anchor bins of every count

    def anchor(position, start, end):            # GetAnchorType(alignmentEndPosition, basePosition, alignmentStartPosition)
        left, right = position - start, end - position
        if left >= right:
            return np.where(right >= ANCHOR_SIZE, ANCHOR_SIZE, NUM_ANCHORS - right - 1)
        return np.where(left >= ANCHOR_SIZE, ANCHOR_SIZE, left)

    def anchors(position, start, end):
        position = np.asarray(position, np.int64)
        left, right = position - start, end - position
        return np.where(left >= right, np.where(right >= ANCHOR_SIZE, ANCHOR_SIZE, NUM_ANCHORS - right - 1), np.where(left >= ANCHOR_SIZE, ANCHOR_SIZE, left))

    def check_deletion_quality(q, i):            # CandidateVariantFinder.CheckDeletionQuality
        if len(q) == 0:
            return False
        after = q[i] if i < len(q) else q[i - 1]
        before = q[i - 1] if i > 0 else after
        return before >= min_bq and after >= min_bq

    for rd in reads:
        cigar, q, start = rd["cigar"], np.asarray(rd["quals"], np.int64), rd["pos"]
        seq = np.frombuffer(rd["seq"] if isinstance(rd["seq"], bytes) else rd["seq"].encode(), np.uint8)
        n = len(seq)
        dirs = np.asarray(rd["dirs"], np.int64) if rd.get("dirs") is not None else np.full(n, DIR_REVERSE if rd["reverse"] else DIR_FORWARD, np.int64)
        pm, rp = np.full(n, -1, np.int64), start                                   # Read.PositionMap
        ri = 0
        for op, l in cigar:
            if op in ALIGNED_OPS:
                pm[ri:ri + l] = np.arange(rp, rp + l)
            if op in REF_OPS:
                rp += l
            if op in READ_OPS:
                ri += l
        end = start + ref_span_of(cigar) - 1                                       # Read.EndPosition
        ends_del = len(cigar) >= 1 and cigar[-1][0] == "D"
        ends_del_soft = len(cigar) >= 2 and cigar[-2][0] == "D" and cigar[-1][0] == "S"
        mapped = np.flatnonzero(pm >= 0)
        # the bases
        allele = np.array([ALLELE_OF.get(int(b), ALLELE_N) for b in seq[mapped]], np.int64)
        allele[q[mapped] < min_bq] = ALLELE_N
        P.append(pm[mapped]); A.append(allele); D.append(dirs[mapped]); AN.append(anchors(pm[mapped], start, end))
        # the gaps: positions between the position mapped last and this base's
        last = np.concatenate([[start - 1], pm[mapped][:-1]]) if len(mapped) else np.zeros(0, np.int64)
        for j in np.flatnonzero(pm[mapped] > last + 1):
            i = int(mapped[j])
            if check_deletion_quality(q, i):
                gap = np.arange(last[j] + 1, pm[i])
                P.append(gap); A.append(np.full(len(gap), ALLELE_DEL)); D.append(np.full(len(gap), dirs[i]))
                AN.append(np.full(len(gap), anchor(pm[i], start, end)))
        last_position = int(pm[mapped][-1]) if len(mapped) else start - 1
        if ends_del_soft:
            del_len, before = cigar[-2][1], n - cigar[-1][1]
            # (the loop reaches index `before`, the first soft-clipped base, with lastPosition = the last mapped position before it)
            lp = int(pm[mapped[mapped < before]][-1]) if (mapped < before).any() else start - 1
            if 0 <= before < n and check_deletion_quality(q, before):
                run = lp + np.arange(1, del_len + 1)
                P.append(run); A.append(np.full(del_len, ALLELE_DEL)); D.append(np.full(del_len, dirs[before])); AN.append(np.full(del_len, NUM_ANCHORS - 1))
        if ends_del and n > 0 and check_deletion_quality(q, n - 1):
            del_len = cigar[-1][1]
            run = last_position + np.arange(1, del_len + 1)
            P.append(run); A.append(np.full(del_len, ALLELE_DEL)); D.append(np.full(del_len, dirs[n - 1])); AN.append(np.full(del_len, NUM_ANCHORS - 1))
    out = np.zeros(region_loci * 6 * 3 * NUM_ANCHORS, np.int64)
    if P:
        p, a, dd, an = (np.concatenate(x).astype(np.int64) for x in (P, A, D, AN))
        inside = (p >= region_start) & (p < region_start + region_loci)
        cell = (((p - region_start) * 6 + a) * 3 + dd) * NUM_ANCHORS + an
        out += np.bincount(cell[inside], minlength=len(out))
    return out.astype(np.int32).reshape(region_loci, 6, 3, NUM_ANCHORS)


def oracle_tensor(reads, region_start, region_loci, min_bq=20):
    from tests import orc
    st = orc.State(region_start, region_loci, min_bq=min_bq)
    for rd in reads:
        assert st.add_allele_counts(orc.make_read(rd["pos"], rd["seq"], cigar=rd["cigar"], quals=rd["quals"], reverse=rd["reverse"], dirs=rd.get("dirs"))) == 0
    return st.counts()


def runs_of_keys(keys):
    """[(first position, loci)] of the runs of consecutive blocks among `keys`."""
    out = []
    for key in keys:
        if out and out[-1][2] == key - 1:
            out[-1][2] = key
        else:
            out.append([key, key, key])
    return [((a - 1) * BLOCK + 1, (c - a + 1) * BLOCK) for a, _, c in out]


def config(which):
    """The two configurations the grid runs under.  "default": min_coverage 1, low_depth_filter 1.  "every allele a row":
    min_variant_qscore 0 and min_frequency 0 as well — pisces_hip_create checks abi_version, tile_loci, the three enums, block_size and
    min_base_call_quality and takes min_frequency as it is (make_params), so 0 is the lowest value that means anything: an allele with
    one read is then callable (the test is `frequency < min_frequency`)."""
    from pisces_amd import _abi
    if which == "default":
        return _abi.default_config(min_coverage=1, low_depth_filter=1)
    assert which == "every allele a row"
    return _abi.default_config(min_coverage=1, low_depth_filter=1, min_variant_qscore=0, min_frequency=0.0)


CONFIGS = ("default", "every allele a row")
NO_ORACLE_ROWS = ("fields by D",)      # deletions of 65 000 bases: beyond the oracle's candidate records; the count tensor judges the flush there


def oracle_rows(scene, which):
    """(records, allele strings) of the oracle running the scene's schedule."""
    from tests import orc
    key = ("rows", scene.name, which)
    assert scene.name not in NO_ORACLE_ROWS
    if key not in _CACHE:
        ups = [u for u in scene.ups if u is not None]
        if ups:
            rows, alleles, _ = orc.run_reads_schedule(read_batch(scene.reads), scene.ref, 1, scene.n_loci, config(which), ups)
        else:       # (one final batch: the same rows without the schedule's working set of allele strings, None here)
            rows, alleles = orc.run_reads(read_batch(scene.reads), scene.ref, 1, scene.n_loci, config(which))[0], None
        _CACHE[key] = (rows, alleles)
    return _CACHE[key]


def rows_agree_with_tensor(rows, tensor, ref, region_start=1):
    """The oracle's rows against the count tensor folded over anchors (tuple_geometry.rows_agree_with_tensor for reads)."""
    from tests import tuple_geometry as tg
    return tg.rows_agree_with_tensor(rows, tensor, ref, region_start)
