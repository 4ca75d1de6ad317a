"""RegionMapper's padding as a closed form, against the host formatter (engine.format_vcf with pad=...).

A writer that pads on the device (not in yet) cannot walk the mapper's cursors position by position: it needs, for a
whole call, the SET of pad positions and the three words of PiscesVcfPadState afterwards.  closed_form() below states both in plain
Python, with no code of the library; the host formatter, pinned to the lines Pisces wrote by tests/test_vcf_format.py, is the authority.

The closed form, for a state (W, L, C) = (last_variant_position_written, last_padded_position, last_cleared_interval_index) that the
API or zero-initialisation produced, and rows in non-descending position order:
  * a line is written per row, or with crush per run of equal positions (its "head");
  * in front of a head at P, with W the position written last (the state's word for the first head of a call, the head before it
    otherwise), the pad rows are the interval positions q, of intervals behind index C, with max(W, L) + 1 <= q <= P - 1;
  * with finish the same range behind the last line is open-ended, and W becomes 0;
  * L is the last pad position, W the last line's position;
  * C ends as max(C, (number of intervals whose end < S) - 1) where S - 1 is the position written last when the host makes its last
    GetNextEmptyCall of the call — which it makes in front of a head only when W == 0 or W + 1 < P, and always with finish."""
import numpy as np

from pisces_amd import _abi, engine


def closed_form(state, intervals, positions, finish, crush):
    """(pad positions in order of writing, (W, L, C) afterwards) of one call"""
    W, L, C = state
    behind = [q for k, (a, b) in enumerate(intervals) if k > C for q in range(a, b + 1)]
    pads = []
    heads = [p for k, p in enumerate(positions) if not crush or k == 0 or p != positions[k - 1]]
    gaps = [(P - 1, True) for P in heads] + ([(None, False)] if finish else [])
    for k, (hi, is_head) in enumerate(gaps):
        asked = not is_head or W == 0 or W + 1 < hi + 1
        gap = [q for q in behind if q >= max(W, L) + 1 and (hi is None or q <= hi)]
        assert asked or not gap
        pads += gap
        if gap:
            W = L = gap[-1]
        if asked:
            C = max(C, sum(1 for (a, b) in intervals if b < W + 1) - 1)
        if is_head:
            W = heads[k]
    if finish:
        W = 0
    return pads, (W, L, C)


def rows_at(positions):
    r = np.zeros(len(positions), dtype=_abi.CALLED_ALLELE_DTYPE)
    r["position"] = positions
    r["total_coverage"], r["allele_support"], r["reference_support"] = 100, 40, 60   # DP=100: no row looks like a pad row
    r["info"] = 2 | (0 << 4) | (0 << 7) | (3 << 10)                                  # 0/1, SNV, A>T
    r["strand_bias_score"] = 0.5
    return r


def draw(rng):
    n_iv = int(rng.integers(0, 41)) if rng.integers(0, 4) else int(rng.integers(0, 4))
    intervals, at = [], 1 if rng.integers(0, 3) == 0 else int(rng.integers(1, 6))   # a third of the sets start at position 1
    for _ in range(n_iv):
        length = 1 if rng.integers(0, 3) == 0 else int(rng.integers(2, 9))
        intervals.append((at, at + length - 1))
        at += length + (0 if rng.integers(0, 3) == 0 else int(rng.integers(1, 7)))   # adjacent: end + 1 == next start
    top = (intervals[-1][1] if intervals else 10) + 4
    marks = sorted({1, top} | {x for a, b in intervals for x in (a - 1, a, b, b + 1) if x >= 1})
    k = int(rng.integers(0, 25))
    pos = [int(marks[int(rng.integers(0, len(marks)))]) if rng.integers(0, 2) else int(rng.integers(1, top + 1)) for _ in range(k)]
    pos += [p for p in pos if rng.integers(0, 3) == 0] + [p for p in pos if rng.integers(0, 6) == 0]   # several per position
    pos.sort()
    n_calls = int(rng.integers(1, 5))
    cuts = sorted(int(rng.integers(0, len(pos) + 1)) for _ in range(n_calls - 1))   # equal cuts: empty calls in between
    ref_len = max(1, top - int(rng.integers(0, 12))) if rng.integers(0, 2) else top + 3   # shorter than the last interval, or not
    return intervals, pos, [0] + cuts + [len(pos)], ref_len, int(rng.integers(0, 2))


def test_the_closed_form_is_what_the_host_formatter_pads():
    rng = np.random.default_rng(20261019)
    seen = dict(pads=0, empty_calls=0, adjacent=0, beyond_reference=0, crush=0, at_one=0)
    for d in range(2500):
        intervals, pos, cuts, ref_len, crush = draw(rng)
        reference = bytes(rng.integers(0, 4, ref_len).astype(np.uint8).choose(np.frombuffer(b"ACGT", dtype=np.uint8)))
        state = engine.new_pad_state()
        mine = (0, 0, -1)
        for c in range(len(cuts) - 1):
            part = pos[cuts[c]:cuts[c + 1]]
            finish = c == len(cuts) - 2
            text = engine.format_vcf("chr1", rows_at(part), crush=crush, pad=dict(state=state, reference=reference, intervals=intervals, finish=finish))
            lines = [l.split("\t") for l in text.split("\n")[:-1]]
            host_pads = [(int(f[1]), f[3]) for f in lines if f[7] == "DP=0"]
            pads, mine = closed_form(mine, intervals, part, finish, crush)
            assert [q for q, _ in host_pads] == pads, (d, c, intervals, part, finish, crush)
            assert all(base == (chr(reference[q - 1]) if q <= ref_len else "N") for q, base in host_pads)
            got = (state.last_variant_position_written, state.last_padded_position, state.last_cleared_interval_index)
            assert got == mine, (d, c, intervals, part, finish, crush, got, mine)
            heads = len(set(part)) if crush else len(part)
            assert len(lines) == heads + len(pads)
            seen["pads"] += len(pads)
            seen["empty_calls"] += not part
            seen["beyond_reference"] += any(q > ref_len for q in pads)
        seen["adjacent"] += any(a[1] + 1 == b[0] for a, b in zip(intervals, intervals[1:]))
        seen["crush"] += crush
        seen["at_one"] += bool(intervals) and intervals[0][0] == 1
    assert all(v > 100 for v in seen.values()), seen


def test_a_finished_state_pads_nothing_more_over_the_same_intervals():
    """What the API leaves after finish is (0, L, n - 1): the writer of the next chromosome starts from new_pad_state(), and a caller who
    goes on with the finished one gets rows and no pad rows, from the closed form as from the host."""
    intervals = [(2, 3), (6, 8), (10, 11)]
    state = engine.new_pad_state()
    engine.format_vcf("chr1", rows_at([7]), pad=dict(state=state, reference=b"C" * 15, intervals=intervals, finish=True))
    mine = (state.last_variant_position_written, state.last_padded_position, state.last_cleared_interval_index)
    assert mine == (0, 11, 2)
    text = engine.format_vcf("chr1", rows_at([5, 9]), pad=dict(state=state, reference=b"C" * 15, intervals=intervals, finish=False))
    pads, mine = closed_form(mine, intervals, [5, 9], False, 0)
    assert pads == [] and text.count("\n") == 2
    assert (state.last_variant_position_written, state.last_padded_position, state.last_cleared_interval_index) == mine == (9, 11, 2)
