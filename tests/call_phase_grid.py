"""A directed grid of (support, coverage, strand split) for the call phase — TEST INFRASTRUCTURE, no tests here.

Every streaming-rate kernel computes the variant q-score, the three strand-bias statistics and the somatic genotype q-score in one of
three ways (pisces_amd/csrc/device_math.hip.h): a memo-table hit (support < 256, coverage < 8192, non-allele observations + 1 < 32), a
proved early-out from a logarithm-free bound, or the full FP64 evaluation kept out of line.  The loci below straddle each of those
decisions on purpose; tests/test_call_phase_grid.py holds all three paths to the oracle on them.

The grid is a table of loci with counts by (allele, direction).  From it come
  tuples_of()    the bucketed tuple stream + PiscesTile array of pisces_hip_call_tiles, and the matching (positions, tuples),
  oracle_rows()  the oracle's rows from the same counts set into an orc.State (no tuple is walked: exact and cheap),
  reads_of()     a read batch, one tile per coverage column, for the read store and the candidate kernel,
  regimes()      which of the three paths every called allele takes — a restatement of the predicates and the table bounds in Python
                 that exists only so that the tests can prove what they exercised.  Expected values never come from it.
"""
import math

import numpy as np

from pisces_amd import _abi
from tests import orc

TILE = 64
START = 1001                 # position of locus 0
ANCHOR = _abi.ANCHOR_SIZE    # every observation is well anchored
Q_HI, Q_LO = 37, 12          # a base at Q_LO is below every MinimumBaseCallQuality in use: it counts under N
# reads_of(mixed_quality=True) (NoiseModel.Window): the quality of a base by (alternate?, direction of the read), so that a locus' mean
# error is a mixture and its noise level (int)PtoQ(mean) does not sit on an integer edge, where the order of the additions could decide
Q_MIXED = ((37, 35), (30, 33))
MAX_OBSERVATIONS = 16_000_000   # 64 MB of tuples

# the bounds of the memo tables (pisces_hip_create): support x coverage of vq_tab / sb_tab, coverage of sb0_tab, and
# (non-allele observations + 1) x coverage of gq_tail / gq_cap
TAB_K, TAB_COV, GQ_A = 256, 8192, 32

SHALLOW_COLUMNS = (255, 256, 257, 2000)
DEEP_COLUMNS = (8191, 8192, 8193, 16383, 16384, 20000, 32768, 65536, 70001)
TWO_TILE_COLUMNS = (8192, 20000)
REDUCED_COLUMNS = (8191, 8192, 20000)      # the columns of the table-less kernels and the counts-fed call phase
READ_COLUMNS = (48, 8191, 8192, 20000)
PICK_NOISE, PICK_CAP = 20, 100             # the configuration the supports of the columns are picked for

# Loci dropped BY NAME because one of their rows is tie-prone in one of the configurations of the test (see tie_prone()): a raw
# q-score within 1e-9 of a half-integer, or a bias score within 1e-6 relative of the threshold — there a last-bit difference between
# the device's and the host's log / exp / pow could move an integer and the comparison would test the libm, not the kernel.
# (name, reason); tests/test_call_phase_grid.py asserts that the grid without them has no tie-prone row and that they are few.
DROPPED = []

_BASES = "ACGT"
_CODE = {"A": _abi.ALLELE_A, "C": _abi.ALLELE_C, "G": _abi.ALLELE_G, "T": _abi.ALLELE_T}


def ref_letter(position):
    return _BASES[position % 4]


def alt_letter(position, i=0):
    """The i-th alternate of a position: never the reference base, never a homopolymer with its neighbours (no RMxN filter)."""
    return _BASES[(position + 1 + i) % 4]


# ------------------------------------------------------------------------------------------------------------------------------------
# The predicates of device_math.hip.h, restated (math.frexp for ilogb).  Used to PICK supports and to CLASSIFY rows, never for values.
# ------------------------------------------------------------------------------------------------------------------------------------
_LN2_TRUNC = 0.6931471805


def _ilogb(x):
    return math.frexp(x)[1] - 1


def _ln_ratio_lower_bound(a, x):
    return float(_ilogb(a) - _ilogb(x) - 1) * _LN2_TRUNC


def err_q(noise_level):
    return float(orc.lib.orc_q_to_p(float(noise_level)))          # MathOperations.QtoP(NL)


def err_sb(noise_level):
    return math.pow(10.0, float(np.float32(-1 * noise_level) / np.float32(10.0)))   # Math.Pow(10, -1*NL/10f)


def vq_early_out(k, cov, noise_level, cap):
    """poisson_qscore_try's division-free proof of "the clamp returns the cap"."""
    lam = err_q(noise_level) * cov
    if not (cap <= 110 and k >= 3 and float(k) >= 2.0 * lam):
        return False
    km1 = float(k - 1)
    need = (float(cap) + 1.0) * 0.23025850929940458 + 1e-3
    return km1 * (_ln_ratio_lower_bound(km1, lam) - 1.0) >= need


def vq_regime(k, cov, noise_level, cap, tables=True):
    if k <= 0 or cov <= 0:
        return "zero"
    if tables and k < TAB_K and cov < TAB_COV:
        return "table"
    return "early" if vq_early_out(k, cov, noise_level, cap) else "cold"


def sb_regime(s, c, noise_level, model, tables=True):
    """sb_stats_try for one of the three statistics (overall / forward / reverse)."""
    if s == 0:
        if model == _abi.SB_POISSON:
            return "const"
        return "table" if tables and 0 <= c < TAB_COV else "cold"
    if tables and 0 < s < TAB_K and 0 <= c < TAB_COV:
        return "table"
    a, x = float(s), float(c) * err_sb(noise_level)
    if x > 0.0 and 2.0 * x <= a and a * (_ln_ratio_lower_bound(a, x) - 1.0) + x > 51.0:
        return "early"
    return "cold"


def _gq_terms(support, cov, target_lod):
    """The float32 arithmetic of SomaticGenotypeQualityCalculator.cs:30-33."""
    f = np.float32(support) / np.float32(cov)
    f = f if f < np.float32(1.0) else np.float32(1.0)
    non = np.float32((np.float32(1.0) - f) * np.float32(cov))
    expected = np.float32(np.float32(target_lod) * np.float32(cov))
    return non, expected


def gq_regime(genotype, vq, support, cov, cfg, tables=True, gq_table=True):
    """somatic_gq_try / somatic_gq_tail: `gq_cap` and `gq_tail` are the two memo tables, `floor` and `plain` need neither."""
    if cov == 0 or genotype in (_abi.GT_ALT12_LIKE_NOCALL, _abi.GT_ALT_LIKE_NOCALL, _abi.GT_REF_LIKE_NOCALL):
        return "plain"
    if genotype not in (_abi.GT_HOM_REF, _abi.GT_HOM_ALT):
        return "plain"
    non, expected = _gq_terms(support, cov, cfg.target_lod_frequency)
    if non >= expected:
        return "floor"
    ai = int(float(non) + 1.0)
    if gq_table and 1 <= ai < GQ_A and cov < TAB_COV:
        return "gq_cap" if tables and vq == cfg.max_variant_qscore else "gq_tail"
    return "cold"


# ------------------------------------------------------------------------------------------------------------------------------------
# The grid
# ------------------------------------------------------------------------------------------------------------------------------------
class Grid:
    """names[i], part[i], column[i] (total coverage the locus was made for; 0 in the corner), counts[i, allele type, direction],
    n_alts[i]; positions START + i; tile_edges: loci [tile_edges[t], tile_edges[t + 1]) are tile t (a column never shares a tile)."""

    def __init__(self, loci):
        self.names = [l[0] for l in loci]
        self.part = np.array([l[1] for l in loci])
        self.column = np.array([l[2] for l in loci], np.int64)
        n = len(loci)
        self.n_loci = n
        self.start = START
        self.positions = START + np.arange(n, dtype=np.int64)
        self.counts = np.zeros((n, 6, 3), np.int64)
        self.n_alts = np.zeros(n, np.int64)
        for i, (_, _, _, spec) in enumerate(loci):
            p = START + i
            for role, d, v in spec:
                a = {"ref": _CODE[ref_letter(p)], "N": _abi.ALLELE_N, "D": _abi.ALLELE_DEL}.get(role)
                if a is None:
                    a = _CODE[alt_letter(p, int(role[3:]))]
                    self.n_alts[i] = max(self.n_alts[i], int(role[3:]) + 1)
                assert v >= 0
                self.counts[i, a, d] += v
        edges = [0]
        for i in range(1, n + 1):
            if i == n or (loci[i][1], loci[i][2]) != (loci[i - 1][1], loci[i - 1][2]) or i - edges[-1] == TILE:
                edges.append(i)
        self.tile_edges = np.array(edges, np.int64)
        self.ref = np.frombuffer("".join(ref_letter(p) for p in range(1, START + n + 40)).encode(), dtype=np.uint8).copy()
        self.n_obs = int(self.counts.sum())


def _balanced(k, cov, alt="alt0"):
    """One alternate with support k of cov, forward / reverse balanced (the odd one goes to reverse)."""
    cf, kf = cov // 2, k // 2
    return [(alt, 0, kf), (alt, 1, k - kf), ("ref", 0, cf - kf), ("ref", 1, (cov - cf) - (k - kf))]


def first_support_at_cap(cov, noise_level=PICK_NOISE, cap=PICK_CAP):
    """The smallest support whose oracle q-score is the cap (the q-score rises with the support)."""
    lo, hi = 1, cov
    if orc.lib.orc_poisson_qscore(hi, cov, noise_level, cap) < cap:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if orc.lib.orc_poisson_qscore(mid, cov, noise_level, cap) >= cap:
            hi = mid
        else:
            lo = mid + 1
    return lo


def first_early_out_support(cov, noise_level=PICK_NOISE, cap=PICK_CAP):
    for k in range(3, cov + 1):
        if vq_early_out(k, cov, noise_level, cap):
            return k
    return None


def column_supports(cov, room, low=False):
    """The supports of a coverage column, most wanted first, cut to `room`: the cap edge, the early-out edge, the support edge of the
    tables, cov - n (hom-alt / hom-ref with non-allele observations across 31 / 32 / 33 and across target_lod * cov), cov // 2, and
    then supports spread through the cold range and up to the early-out.  low: the supports 8 .. 64 too, where the cap and the
    early-out of the lower noise levels (30, 37) lie at this depth."""
    cap_k, early_k = first_support_at_cap(cov), first_early_out_support(cov)
    picks = []
    if cap_k is not None:
        picks += [cap_k - 1, cap_k]
    if early_k is not None:
        picks += [early_k - 1, early_k]
    picks += [254, 255, 256, 257]
    picks += [cov - n for n in range(36)]
    picks += [cov // 2]
    lam = cov / 100.0
    top = early_k if early_k is not None else cov
    picks += [int(round(lam * f)) for f in (0.5, 0.6, 0.7, 0.8, 0.9, 0.98)]     # hom-ref rows with a LowGQ genotype q-score
    if low:
        picks += list(range(8, 41)) + list(range(44, 66, 4))
    if cap_k is not None:
        step = max((top - cap_k) // 12, 1)
        picks += list(range(cap_k + 1, top, step))                               # cold, at the cap
        step = max((cap_k - int(lam)) // 12, 1)
        picks += list(range(int(lam) + 1, cap_k, step))                          # cold, below the cap
    picks += list(range(1, 8))
    picks += [top + 1, top + 7, 2 * top, 3 * top]
    out = []
    for k in picks:
        if 1 <= k <= cov and k not in out:
            out.append(k)
    return out[:room]


def _corner():
    return [("corner/k%d/c%d" % (k, cov), "corner", 0, _balanced(k, cov)) for cov in range(1, 49) for k in range(1, cov + 1)]


def _columns():
    loci = []
    for cov in SHALLOW_COLUMNS:
        ks = list(range(1, 41)) + list(range(250, 261)) + [cov // 2] + [cov - n for n in range(36)]
        if cov == 2000:
            ks += list(range(60, 700, 12)) + [first_support_at_cap(cov) - 1, first_support_at_cap(cov)]
        for k in sorted({k for k in ks if 1 <= k <= cov}):
            loci.append(("c%d/k%d" % (cov, k), "column", cov, _balanced(k, cov)))
    for cov in DEEP_COLUMNS:
        room = 2 * TILE if cov == 8192 else 96 if cov == 20000 else TILE if cov <= 16384 else 48   # (the observation budget)
        for k in sorted(column_supports(cov, room, low=cov in (8192, 8193, 20000))):
            loci.append(("c%d/k%d" % (cov, k), "column", cov, _balanced(k, cov)))
    return loci


def _layouts():
    """Strand layouts on the columns 2000, 8192, 16384 and 20000."""
    loci = []

    def add(name, cov, spec):
        loci.append(("s%d/%s" % (cov, name), "layout", cov, spec))

    for cov in (2000, 8192, 16384, 20000):
        cap_k = first_support_at_cap(cov)
        for k in (5, cap_k - 1, cap_k + 40):
            # all forward: cov_both is false, the bias score is 0
            add("fwd/k%d" % k, cov, [("alt0", 0, k), ("ref", 0, cov - k)])
            # the support on one strand only, the coverage on both
            add("sup_fwd/k%d" % k, cov, [("alt0", 0, k), ("ref", 0, cov // 2 - k), ("ref", 1, cov - cov // 2)])
            add("sup_rev/k%d" % k, cov, [("alt0", 1, k), ("ref", 0, cov // 2), ("ref", 1, cov - cov // 2 - k)])
            # odd stitched support and odd stitched coverage: the per-strand statistics take the integer halves
            st = 2 * (cov // 6) + 1
            ks = min(k, st) | 1
            rest, krest = cov - st, max(k - ks, 0)
            add("stitched/k%d" % k, cov, [("alt0", 2, ks), ("ref", 2, st - ks), ("alt0", 0, krest // 2), ("alt0", 1, krest - krest // 2),
                                          ("ref", 0, rest // 2 - krest // 2), ("ref", 1, rest - rest // 2 - (krest - krest // 2))])
        # a stitched-only locus: F = S / 2 = R
        add("stitched_only", cov, [("alt0", 2, 301), ("ref", 2, cov - 301)])
    # a per-strand coverage of exactly 8191 and exactly 8192 (the coverage edge of the per-strand table index)
    for cf, cr in ((8191, 8191), (8191, 8192), (8192, 8191), (8192, 8192), (8191, 300), (300, 8192)):
        for kf, kr in ((3, 2), (120, 100), (255, 256), (0, 90), (200, 0)):
            add("strands_%d_%d/k%d_%d" % (cf, cr, kf, kr), cf + cr, [("alt0", 0, kf), ("alt0", 1, kr), ("ref", 0, cf - kf), ("ref", 1, cr - kr)])
    # ... and reached through the stitched half: F + S/2 = 8191 / 8192
    for s in (4001, 4002):
        add("half_%d" % s, 6191 + 6000 + s, [("alt0", 0, 60), ("alt0", 2, 41), ("alt0", 1, 50), ("ref", 0, 6131), ("ref", 1, 5950), ("ref", 2, s - 41)])
    for cov in (2000, 8192, 20000):
        t = cov // 100
        # three alternates (the multi-allelic site of the somatic caller: four rows a locus)
        add("three_alts", cov, _balanced(6 * t, cov)[2:] + _balanced(3 * t, 3 * t, "alt0")[:2] + _balanced(2 * t, 2 * t, "alt1")[:2]
            + _balanced(t, t, "alt2")[:2])
        add("three_alts_low", cov, _balanced(7, cov)[2:] + [("alt0", 0, 2), ("alt0", 1, 2), ("alt1", 0, 2), ("alt2", 1, 1)])
        # low-quality bases count under N: no-calls next to the coverage
        add("with_n", cov, _balanced(2 * t, cov) + [("N", 0, cov // 3), ("N", 1, cov // 5)])
        add("mostly_n", cov, _balanced(2, 40) + [("N", 0, cov - 40)])
        # deletion tuples count as coverage and never as support
        add("with_del", cov, _balanced(2 * t, cov - 3 * t) + [("D", 0, t), ("D", 1, 2 * t)])
        add("del_only_fwd", cov, [("D", 0, cov // 2), ("ref", 1, cov - cov // 2 - 3), ("alt0", 1, 3)])
    # no alternate at all: a Reference row stays (a called variant takes its locus' Reference row away), hom-ref with the deletions as its
    # non-allele observations — across 31 / 32 / 33, and close under target_lod * cov, where the genotype q-score is low (LowGQ)
    for cov in (2000, 8192, 16384, 20000):
        for d in ((5, 30, 31, 32, 33) if cov <= 8192 else (32,)) + (int(0.0085 * cov),):
            add("ref_and_del/d%d" % d, cov, [("D", 0, d // 2), ("D", 1, d - d // 2), ("ref", 0, cov // 2 - d // 2), ("ref", 1, cov - cov // 2 - (d - d // 2))])
    return loci


_GRID = {}


def grid(which="full"):
    """which: "full", or "reduced" (the exhaustive corner and the columns 8191, 8192 and 20000)."""
    key = which
    if key in _GRID:
        return _GRID[key]
    dropped = {n for n, _ in DROPPED}
    loci = [l for l in _corner() + _columns() + _layouts() if l[0] not in dropped]
    assert len({l[0] for l in loci}) == len(loci)
    if which == "reduced":
        loci = [l for l in loci if l[1] == "corner" or (l[1] == "column" and l[2] in REDUCED_COLUMNS)]
    g = Grid(loci)
    if which != "reduced":
        assert g.n_obs < MAX_OBSERVATIONS, g.n_obs   # the whole stream, the deep part (nearly all of it) included
        per_col = {int(c): int(((g.column == c) & (g.part == "column")).sum()) for c in DEEP_COLUMNS}
        assert all(n <= (2 * TILE if c in TWO_TILE_COLUMNS else TILE) for c, n in per_col.items()), per_col
    _GRID[key] = g
    return g


# ------------------------------------------------------------------------------------------------------------------------------------
# The three forms of the same counts
# ------------------------------------------------------------------------------------------------------------------------------------
def _ref_codes(g):
    return np.array([_CODE[ref_letter(int(p))] for p in g.positions], np.int64)


def tuples_of(g, tile=TILE):
    """(stream, tiles, positions, tuples): the bucketed tuple stream (uint32, a pad word first so that segments start unaligned, as in
    test_fused_kernel_edge_inputs) and its PiscesTile array for pisces_hip_call_tiles; positions / tuples: the same observations for
    AddObservations and orc.run_observations.  A low-quality base is a reference base at Q_LO; a deletion carries quality 255."""
    assert tile == TILE
    idx = np.nonzero(g.counts.reshape(-1))[0]
    reps = g.counts.reshape(-1)[idx]
    locus, allele, direction = idx // 18, (idx // 3) % 6, idx % 3
    ref_code = _ref_codes(g)
    packed_allele = np.where(allele == _abi.ALLELE_N, ref_code[locus], allele)
    qual = np.where(allele == _abi.ALLELE_N, Q_LO, np.where(allele == _abi.ALLELE_DEL, 255, Q_HI))
    tile_of_locus = np.searchsorted(g.tile_edges, np.arange(g.n_loci), side="right") - 1
    in_tile = np.arange(g.n_loci) - g.tile_edges[tile_of_locus]
    cell = _abi.tuple_pack(in_tile[locus].astype(np.uint32), np.full(len(idx), ANCHOR, np.uint32), direction.astype(np.uint32),
                           packed_allele.astype(np.uint32), qual.astype(np.uint32)).astype(np.uint32)
    tuples = np.repeat(cell, reps)
    positions = np.repeat(g.positions[locus].astype(np.int32), reps)
    per_locus = g.counts.reshape(g.n_loci, -1).sum(axis=1)
    per_tile = np.add.reduceat(per_locus, g.tile_edges[:-1])
    begin = 1 + np.concatenate([[0], np.cumsum(per_tile)[:-1]])
    tiles = np.zeros(len(g.tile_edges) - 1, dtype=_abi.TILE_DTYPE)
    tiles["start_position"] = g.start + g.tile_edges[:-1]
    tiles["n_loci"] = np.diff(g.tile_edges)
    tiles["tuple_begin"] = begin
    tiles["tuple_end"] = begin + per_tile
    stream = np.concatenate([np.full(1, _abi.TUPLE_PAD, np.uint32), tuples, np.full(3, _abi.TUPLE_PAD, np.uint32)])
    return stream, tiles, positions, tuples


def oracle_rows(g, cfg):
    """The oracle's rows for the grid's counts: the counts set into an orc.State (orc.State.set_count's array, written in one go) at the
    anchor index of the tuples, an SNV candidate for every alternate with support (what the observations of tuples_of would have
    added one by one), then call_all."""
    st = orc.State(g.start, g.n_loci, min_bq=cfg.min_base_call_quality)
    na = orc.lib.orc_num_anchor_indexes(st.h)
    a = np.ctypeslib.as_array(orc.lib.orc_counts_ptr(st.h), shape=(g.n_loci, 6, 3, na))
    a[:, :, :, ANCHOR] = g.counts
    for i in np.nonzero(g.n_alts)[0]:
        p = int(g.positions[i])
        for k in range(int(g.n_alts[i])):
            sup = tuple(int(v) for v in g.counts[i, _CODE[alt_letter(p, k)]])
            if sum(sup):
                rc = st.add_candidate(orc.make_candidate(p, _abi.CAT_SNV, ref_letter(p), alt_letter(p, k), support=sup, well_anchored=sup))
                assert rc == 0
    return st.call_all(g.ref.tobytes(), cfg)


def read_columns(columns=READ_COLUMNS):
    """[(coverage, [support at locus 0..63])]: an alternate at every third locus (no two within an MNV's reach, none on a read end), the
    supports of the column's edges."""
    out = []
    for cov in columns:
        if cov >= 8191:
            # the cap pair, the early-out pair, 254 .. 257; hom-alt across 31 / 32 / 33; half; just under 1 % (left uncalled by a
            # frequency threshold there: a LowGQ hom-ref row); a few supports where the lower noise levels of the Window model decide
            pri = column_supports(cov, 8) + [cov - n for n in (0, 1, 30, 31, 32, 35)] + [cov // 2, int(0.009 * cov), 4, 9, 14, int(0.013 * cov)]
        else:
            pri = [1, 2, 3, 5, 8, 12, 16, 20, cov, cov - 1, 18, 17, 13, 24, 30, 36, 40, 44, 46, 7]
        ks = []
        for k in pri:
            if 1 <= k <= cov and k not in ks:
                ks.append(k)
        sup = [0] * TILE
        for j, l in enumerate(range(2, TILE - 2, 3)):
            sup[l] = ks[j % len(ks)]
        out.append((cov, sup))
    return out


def reads_of(columns=READ_COLUMNS, corner=False, mixed_quality=False):
    """(ReadBatch, ref, [(coverage, first position, supports)]): one tile per coverage column — `cov` reads of 64 bases, all starting
    at the tile's first locus; the alternate base at locus l sits in the first k_l reads; directions go by read (odd reads reverse).
    corner: behind the columns, every (k, cov) of the exhaustive corner as `cov` reads of three bases with the alternate in the middle of
    the first k (three positions a locus: no read touches the next locus).  mixed_quality: base qualities Q_MIXED by (alternate?,
    direction of the read) for NoiseModel.Window; the corner then starts at coverage 2 (one read has one quality: its noise level sits
    on the integer edge of PtoQ)."""
    cols = read_columns(columns)
    first_corner = START + TILE * len(cols) + 8
    corner_loci = [(k, cov) for cov in range(2 if mixed_quality else 1, 49) for k in range(1, cov + 1)] if corner else []
    ref = np.frombuffer("".join(ref_letter(p) for p in range(1, first_corner + 3 * len(corner_loci) + 40)).encode(), dtype=np.uint8).copy()
    pos, flags, bases, quals, lens, layout = [], [], [], [], [], []

    def add(first, width, cov, sup):
        row_ref = np.frombuffer("".join(ref_letter(first + l) for l in range(width)).encode(), dtype=np.uint8)
        row_alt = np.frombuffer("".join(alt_letter(first + l) for l in range(width)).encode(), dtype=np.uint8)
        m = np.arange(cov)[:, None] < np.array(sup)[None, :]
        rev = (np.arange(cov) % 2).astype(np.uint8)
        bases.append(np.where(m, row_alt[None, :], row_ref[None, :]).astype(np.uint8).reshape(-1))
        q = np.array(Q_MIXED, np.uint8)[m.astype(np.int64), rev[:, None].astype(np.int64)] if mixed_quality else np.full(m.shape, Q_HI, np.uint8)
        quals.append(q.reshape(-1))
        pos.append(np.full(cov, first, np.int32))
        flags.append(rev)
        lens.append(np.full(cov, width, np.int64))

    for t, (cov, sup) in enumerate(cols):
        add(START + t * TILE, TILE, cov, sup)
        layout.append((cov, START + t * TILE, sup))
    for j, (k, cov) in enumerate(corner_loci):
        add(first_corner + 3 * j, 3, cov, [0, k, 0])
        layout.append((cov, first_corner + 3 * j, [0, k, 0]))
    lens = np.concatenate(lens)
    n = len(lens)
    batch = _abi.ReadBatch.from_arrays(position=np.concatenate(pos), flags=np.concatenate(flags), cigar_offset=np.arange(n + 1, dtype=np.int32),
                                       cigar_op=np.full(n, ord("M"), np.uint8), cigar_len=lens.astype(np.uint32),
                                       seq_offset=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), bases=np.concatenate(bases),
                                       quals=np.concatenate(quals))
    return batch, ref, layout


def window_level_margin_of_reads(batch):
    """Per covered position, the distance of the Window model's raw noise level -10 log10(mean error) from the nearest integer."""
    lens = np.diff(batch.seq_offset)
    p = np.repeat(batch.position.astype(np.int64) - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(len(batch.quals))
    err = np.bincount(p, weights=np.power(10.0, -batch.quals.astype(np.float64) / 10.0))
    cov = np.bincount(p)
    level = -10.0 * np.log10(err[cov > 0] / cov[cov > 0])
    return np.abs(level - np.rint(level))


# ------------------------------------------------------------------------------------------------------------------------------------
# What the rows exercise
# ------------------------------------------------------------------------------------------------------------------------------------
def regimes_of_rows(rows, cfg, tables=True, gq_table=True):
    """Per row: (variant q-score regime, [overall, forward, reverse strand-bias regime], genotype q-score regime)."""
    out = []
    nl, cap, model = cfg.noise_level, cfg.max_variant_qscore, cfg.strand_bias_model
    for r in rows:
        k, cov = int(r["allele_support"]), int(r["total_coverage"])
        cd, sd = [int(v) for v in r["coverage_by_dir"]], [int(v) for v in r["support_by_dir"]]
        vq = vq_regime(k, cov, nl, cap, tables) if cov else "zero"
        if k > 0:
            sb = [sb_regime(sum(sd), sum(cd), nl, model, tables), sb_regime(sd[0] + sd[2] // 2, cd[0] + cd[2] // 2, nl, model, tables),
                  sb_regime(sd[1] + sd[2] // 2, cd[1] + cd[2] // 2, nl, model, tables)]
        else:
            sb = ["none"] * 3
        gq = gq_regime(int(_abi.info_genotype(int(r["info"]))), int(r["variant_qscore"]), k, cov, cfg, tables, gq_table)
        out.append((vq, sb, gq))
    return out


def regimes(g, cfg, tables=True, gq_table=True):
    """Counts of the called alleles of the grid by regime: {"vq": {...}, "vq_cold_below_cap": n, "vq_cold_at_cap": n,
    "sb_overall" / "sb_forward" / "sb_reverse": {...}, "gq": {...}}."""
    rows = oracle_rows(g, cfg)
    per = regimes_of_rows(rows, cfg, tables, gq_table)
    out = {"vq": {}, "sb_overall": {}, "sb_forward": {}, "sb_reverse": {}, "gq": {}, "vq_cold_below_cap": 0, "vq_cold_at_cap": 0, "rows": len(rows)}
    for r, (vq, sb, gq) in zip(rows, per):
        out["vq"][vq] = out["vq"].get(vq, 0) + 1
        if vq == "cold":
            out["vq_cold_at_cap" if int(r["variant_qscore"]) == cfg.max_variant_qscore else "vq_cold_below_cap"] += 1
        for name, v in zip(("sb_overall", "sb_forward", "sb_reverse"), sb):
            out[name][v] = out[name].get(v, 0) + 1
        out["gq"][gq] = out["gq"].get(gq, 0) + 1
    return out


def tie_prone(g, cfg):
    """[(locus name, reason)] of the rows whose integer could turn on the last bits of a logarithm: the raw variant q-score within 1e-9
    of a half-integer below the cap; the raw genotype q-score -10 log10(QtoP(vq) + PoissonCdf(non-allele, expected)) within 1e-9 of a
    half-integer inside [min_gq, max_gq]; the bias score within 1e-6 relative of the threshold.  From the oracle alone.  (1e-9 is about
    a hundred times what a few ulp of log or exp move a value near 100.)"""
    rows = oracle_rows(g, cfg)
    out = []
    thr = float(cfg.strand_bias_threshold)
    for r in rows:
        name = g.names[int(r["position"]) - g.start]
        k, cov = int(r["allele_support"]), int(r["total_coverage"])
        if k > 0 and cov > 0 and cfg.noise_model == 0:
            raw = float(orc.lib.orc_raw_poisson_qscore(k, cov, cfg.noise_level))
            if raw < cfg.max_variant_qscore + 0.5 and abs((raw % 1.0) - 0.5) < 1e-9:
                out.append((name, "raw variant q-score %.12f" % raw))
        gt = int(_abi.info_genotype(int(r["info"])))
        if cov > 0 and gt in (_abi.GT_HOM_REF, _abi.GT_HOM_ALT):
            non, expected = _gq_terms(k, cov, cfg.target_lod_frequency)
            if non < expected:
                p = float(orc.lib.orc_q_to_p(float(int(r["variant_qscore"])))) + float(orc.lib.orc_poisson_cdf(float(non), float(expected)))
                raw = float(orc.lib.orc_p_to_q(p)) if p > 0 else math.inf
                if cfg.min_genotype_qscore - 0.5 <= raw <= cfg.max_genotype_qscore + 0.5 and abs((raw % 1.0) - 0.5) < 1e-9:
                    out.append((name, "raw genotype q-score %.12f" % raw))
        if k > 0 and _abi.info_category(int(r["info"])) != _abi.CAT_REFERENCE:
            s = float(r["strand_bias_score"])
            if abs(s - thr) <= 1e-6 * thr:
                out.append((name, "bias score %.12g against the threshold %.12g" % (s, thr)))
    return out
