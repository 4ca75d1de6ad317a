"""The register ring of stream_tuples_wave (csrc/kernels.hip.h): a model of the loop restated from its control flow, and the grid of
tests/test_tuple_ring_cpu.py and tests/test_tuple_ring_gpu.py.

The loop: a row is 64 consecutive dwordx4 of the segment's aligned body; rows are dealt in batches of U = PISCES_WAVE_UNROLL (batch b
belongs to wave b % NW); a wave keeps a ring of 2 U register quads, one row each.  Its steps are numbered k' = 0 .. 2 U G - 1 over G
revolutions, step k' uses slot k' % (2 U).  What is irregular sits in front: the first `pad` steps are empty, and the segment's last batch,
when it has fewer than U rows, is the first batch its owner takes, in the last slots of its half of the ring.  Revolution 0 loads (the
head) and decodes under `k' >= pad`; revolutions 0 .. G - 2 refill every slot for the next revolution (whole batches always); revolution
G - 1 only decodes.  G == 1 is the head and its decode alone.  Lanes are masked in the segment's last row only, when it is not whole.

ring_model() names the regime a segment puts each wave in; replay() walks the same index arithmetic (modulo 2^32, clamped, masked) and
returns every dwordx4 a wave decodes, so that the CPU test can hold the arithmetic itself to "every dwordx4 of the body once".
"""
from types import SimpleNamespace

import numpy as np

from tests import tuple_geometry as tg

K = tg.K
U = K.wave_unroll                      # rows per batch
RING = 2 * U                           # slots
ROW = 64                               # dwordx4 per row
M32 = 0xFFFFFFFF

ROWS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49)
# beyond 49 rows: with two waves a wave has at most four batches (two revolutions) up to there, and the refill loop's second and later
# iterations -- the steady state -- never run; 65, 81 and 97 rows give the two-wave form three and four revolutions, 113 both of its waves
# four.  40, 63 and 64 rows are what the two-wave form still lacks below that: wave 0 with the masked row in its last slot behind a
# refill, wave 1 with the short batch in the first half of a refilled ring, wave 0 refilled without an empty step
LONG_ROWS = (40, 63, 64, 65, 81, 97, 113)
REMAINDERS = (0, 1, 63)                # n4 % 64
SEED = tg.SEED + 7


def wave_scalars(n4, nw, wid, u=U):
    """The wave-uniform values the kernel computes before its first load."""
    batch = ROW * u
    rows = (n4 + ROW - 1) // ROW
    nb = (n4 + batch - 1) // batch
    m = (nb - wid + nw - 1) // nw if wid < nb else 0
    part = rows % u
    own = part != 0 and m != 0 and (nb - 1) % nw == wid
    mf = m - int(own)
    g = (m + 1) // 2
    k = mf * u + (part if own else 0)
    pad = g * 2 * u - k if g else 2 * u
    e0 = ((wid + nw * (mf - 2 * g)) * batch) & M32
    e_part = ((nb - 1) * batch - (u - part) * ROW) & M32
    hv_part = 2 * g - m if own else 2
    head0 = e_part if hv_part == 0 else e0
    head1 = e_part if hv_part == 1 else (e0 + nw * batch) & M32
    last_row = (rows - 1) * ROW if n4 % ROW else M32
    return SimpleNamespace(rows=rows, nb=nb, m=m, part=part, own=own, mf=mf, G=g, K=k, pad=pad, e0=e0, head0=head0, head1=head1,
                           last_row=last_row, hv_part=hv_part)


def replay(n4, nw, wid, u=U):
    """Every (dwordx4 index, lane kept) the wave decodes, in order, and every index it loads: the kernel's loop with its arithmetic."""
    s_ = wave_scalars(n4, nw, wid, u)
    batch, ring = ROW * u, 2 * u
    lanes = np.arange(ROW, dtype=np.int64)
    q = [None] * ring                  # slot -> (first dwordx4 of its row, the clamped indices the load read)
    loads, decoded = [], []

    def fetch(s, e):
        assert n4 > 0                  # n4 - 1 is the clamp
        j = np.minimum((e + lanes) & M32, n4 - 1)
        loads.append(j)
        q[s] = (e, j)

    def decode(s, e_given, may_be_last):
        e, j = q[s]
        assert e == e_given            # the row the kernel believes the slot holds (it tests that one against last_row)
        keep = np.ones(ROW, bool)
        if may_be_last and e == s_.last_row:
            keep = lanes < n4 % ROW
        decoded.append((j, keep))
        q[s] = None                    # a slot is decoded once per load

    def slot_off(s):
        return (s // u) * nw * batch + (s % u) * ROW

    def head_row(s):
        return ((s_.head0 if s < u else s_.head1) + (s % u) * ROW) & M32

    for s in range(ring):              # the head
        if s >= s_.pad:
            fetch(s, head_row(s))
    skip, d0, d1, e = s_.pad, s_.head0, s_.head1, s_.e0

    def step(s):
        if s >= skip:
            decode(s, ((d0 if s < u else d1) + (s % u) * ROW) & M32, s % u == u - 1)

    if s_.G >= 2:
        for _ in range(s_.G - 1):
            e = (e + 2 * nw * batch) & M32
            for s in range(ring):
                step(s)
                fetch(s, (e + slot_off(s)) & M32)
            skip, d0, d1 = 0, e, (e + nw * batch) & M32
        for s in range(ring):
            decode(s, (d1 + (u - 1) * ROW) & M32 if s == ring - 1 else q[s][0], s == ring - 1)
    else:
        for s in range(ring):
            step(s)
    assert all(x is None for x in q)   # nothing loaded is left undecoded
    return s_, loads, decoded


def ring_model(begin, end, nw, u=U):
    """Per wave: idle, revolutions (capped at 4: the refill loop runs 0, 1, 2 or more times), the empty steps in front as a class
    (0, 1 .. U-1, U, U+1 .. 2U-1), whether the wave takes the short batch, and where the masked row is decoded."""
    e = tg.ends_model(begin, end)
    waves = []
    for wid in range(nw):
        s = wave_scalars(e.n4, nw, wid, u)
        if s.G == 0:
            waves.append(SimpleNamespace(idle=True, revolutions=0, pad="-", short=False, mask="none", rows=0, refills=0))
            continue
        pad = "0" if s.pad == 0 else "<U" if s.pad < u else "U" if s.pad == u else ">U"
        mask = "none"
        if e.n4 % ROW:
            last_batch_is_mine = (s.nb - 1) % nw == wid
            if s.own:
                mask = "revolution 0, slot %s" % ("U-1" if s.hv_part == 0 else "2U-1")
            elif last_batch_is_mine and s.part == 0:
                mask = "last slot" if s.G >= 2 else "revolution 0, slot 2U-1"
        waves.append(SimpleNamespace(idle=False, revolutions=min(s.G, 4), pad=pad, short=s.own, mask=mask, rows=s.K,
                                     refills=(s.G - 1) * 2 * u))
    rows = (e.n4 + ROW - 1) // ROW
    assert sum(w.rows for w in waves) == rows
    return SimpleNamespace(ends=e, rows=rows, last_row_whole=e.n4 % ROW == 0, waves=waves)


def regimes_of(begin, end, u=U):
    """Per wave of each form, side by side and not as a product (revolution 0 and the last revolution are the same code however often the
    refill loop runs between them; only G == 1, where revolution 0 is decoded by code of its own, is a path apart):
         ("ring1" | "ring2", wave, "revolutions", 0 (idle) .. 4)
         (.., .., "revolution 0", "alone" | "refilled", empty steps in front, takes the short batch, masked slot of revolution 0 or "none")
         (.., .., "last revolution", its last slot masked)                                  when there is one (G >= 2)"""
    out = []
    for nw in (1, 2):
        m = ring_model(begin, end, nw, u)
        for wid, w in enumerate(m.waves):
            form = "ring%d" % nw
            out.append((form, wid, "revolutions", w.revolutions))
            if w.idle:
                continue
            out.append((form, wid, "revolution 0", "alone" if w.revolutions == 1 else "refilled", w.pad, w.short, w.mask if w.mask != "last slot" else "none"))
            if w.revolutions >= 2:
                out.append((form, wid, "last revolution", w.mask == "last slot"))
    return out


def reachable_regimes(max_rows=max(LONG_ROWS), u=U):
    out = set()
    for n4 in range(0, max_rows * ROW + 1):
        out.update(regimes_of(0, 4 * n4, u))
    return out


def describe(begin, end):
    return "; ".join(" ".join(str(x) for x in r) for r in regimes_of(begin, end))


# ------------------------------------------------------------------------------------------------------------------------------------
# the grid: one tile per (rows, n4 % 64, start alignment)
# ------------------------------------------------------------------------------------------------------------------------------------
def body_dwordx4(rows, rem):
    """n4 of a body of `rows` rows whose last row holds `rem` dwordx4 (0 = it is whole)."""
    if rows == 0:
        return 0
    return ROW * rows if rem == 0 else ROW * (rows - 1) + rem


def grid_cells(rows_list=ROWS + LONG_ROWS):
    """(alignment, length in tuples, rows, remainder): the head is (4 - a) % 4 words; the tail cycles through 0..3 so that a head meets
    no tail, a tail no head, both and neither."""
    cells = []
    for i, rows in enumerate(rows_list):
        for j, rem in enumerate(REMAINDERS if rows else (0,)):
            for a in range(4):
                head, tail = (4 - a) % 4, (a + i + j) % 4
                cells.append((a, head + 4 * body_dwordx4(rows, rem) + tail, rows, rem))
    return cells


def build_grid(seed=SEED):
    key = ("ring grid", K.B, seed)
    if key not in tg._CACHE:
        rng = np.random.default_rng(seed)
        cells = grid_cells()
        segments, loci = [], []
        for _, length, _, _ in cells:
            l, t = tg.draw_tuples(rng, length, tg.TILE)
            loci.append(l)
            segments.append(t)
        g = tg._finish([(a, length) for a, length, _, _ in cells], segments, loci, [tg.TILE] * len(cells), tg.make_reference(rng, tg.TILE * len(cells) + 40))
        g.ring_cells = cells
        tg._CACHE[key] = g
    return tg._CACHE[key]


def cell_name(g, t, layout="guarded"):
    tile = g.layouts[layout][1][t]
    a, length, rows, rem = g.ring_cells[t]
    return "tile %d (a=%d, L=%d, rows=%d, n4 %% 64=%d) [%s] %s" % (t, a, length, rows, rem, layout, describe(int(tile["tuple_begin"]), int(tile["tuple_end"])))
