"""pisces_hip_vcf_pad_plan: the padding of a call without its text.  The entry restates the closed form of tests/test_vcf_pad_cpu.py
with binary searches over the interval table; here it is held to the host formatter itself (pad rows and lines counted in the text,
the state afterwards) on that file's seeded draws, to its refusals, and to a gap no walk over positions could afford."""
import ctypes as C

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import test_vcf_pad_cpu as closed


def words(state):
    return (state.last_variant_position_written, state.last_padded_position, state.last_cleared_interval_index)


def test_the_plan_is_what_the_formatter_then_does():
    rng = np.random.default_rng(20261020)
    pads_seen = calls = 0
    for d in range(2000):
        intervals, pos, cuts, ref_len, crush = closed.draw(rng)
        reference = b"A" * ref_len
        state = engine.new_pad_state()
        mine = (0, 0, -1)
        for c in range(len(cuts) - 1):
            part = closed.rows_at(pos[cuts[c]:cuts[c + 1]])
            finish = c == len(cuts) - 2
            before = words(state)
            pads, lines, after = engine.vcf_pad_plan(part, intervals, state, finish=finish, crush=crush)
            assert words(state) == before                      # the plan leaves the state alone
            text = engine.format_vcf("chr1", part, crush=crush, pad=dict(state=state, reference=reference, intervals=intervals, finish=finish))
            got = [l.split("\t") for l in text.split("\n")[:-1]]
            want_pads, mine = closed.closed_form(mine, intervals, pos[cuts[c]:cuts[c + 1]], finish, crush)
            assert (pads, lines) == (sum(f[7] == "DP=0" for f in got), len(got)), (d, c, intervals, pos, cuts, crush)
            assert words(after) == words(state) == mine, (d, c, intervals, pos, cuts, crush)
            assert pads == len(want_pads)
            pads_seen += pads
            calls += 1
    assert pads_seen > 10_000 and calls > 4000


def test_a_gap_of_two_billion_positions_costs_nothing():
    """one interval over almost every int32 position: the plan is two searches a row, and format_vcf sizes its buffer by the call's own
    no-call rows, not by every position of the interval set"""
    intervals = [(1, 2_000_000_000)]
    state = engine.new_pad_state()
    rows = closed.rows_at([5, 6, 1_000_000_005])
    pads, lines, after = engine.vcf_pad_plan(rows, intervals, state)
    assert (pads, lines, words(after)) == (1_000_000_002, 1_000_000_005, (1_000_000_005, 1_000_000_004, -1))
    pads, lines, after = engine.vcf_pad_plan(rows[:2], intervals, state, finish=True)
    assert (pads, lines, words(after)) == (4 + 2_000_000_000 - 6, 2_000_000_000, (0, 2_000_000_000, 0))
    text = engine.format_vcf("chr1", rows[:2], pad=dict(state=state, reference=b"ACGTACGT", intervals=intervals, finish=False))
    assert [l.split("\t")[1] for l in text.split("\n")[:-1]] == ["1", "2", "3", "4", "5", "6"] and words(state) == (6, 4, -1)


def test_what_the_closed_form_does_not_cover_is_refused():
    intervals = [(2, 3), (6, 8), (10, 11)]
    new = engine.new_pad_state
    for rows, state in [(closed.rows_at([7, 6]), new()),                               # a row below its predecessor
                        (closed.rows_at([0, 6]), new()),                               # a position below 1
                        (closed.rows_at([5, 6]), _abi.PiscesVcfPadState(7, 3, 0)),     # the first row below the position written last
                        (closed.rows_at([9]), _abi.PiscesVcfPadState(5, 7, -1)),       # padded ahead of written, intervals uncleared
                        (closed.rows_at([9]), _abi.PiscesVcfPadState(0, 7, -1)),
                        (closed.rows_at([9]), _abi.PiscesVcfPadState(0, 0, -2))]:
        with pytest.raises(engine.PiscesHipError) as e:
            engine.vcf_pad_plan(rows, intervals, state)
        assert e.value.code == _abi.E_UNSUPPORTED
    for bad in ([(6, 8), (2, 3)], [(2, 6), (6, 8)], [(0, 3)], [(5, 4)]):                # intervals: positive, sorted, disjoint
        with pytest.raises(engine.PiscesHipError) as e:
            engine.vcf_pad_plan(closed.rows_at([9]), bad, new())
        assert e.value.code == _abi.E_INVALID_ARG
    # a finished state is taken and pads nothing more over the same intervals, as the formatter does
    pads, lines, after = engine.vcf_pad_plan(closed.rows_at([5, 9]), intervals, _abi.PiscesVcfPadState(0, 11, 2))
    assert (pads, lines, words(after)) == (0, 2, (9, 11, 2))
    # no intervals, no rows; null outputs
    assert engine.vcf_pad_plan(closed.rows_at([]), [], new(), finish=True)[:2] == (0, 0)
    st = new()
    assert engine.lib.pisces_hip_vcf_pad_plan(None, 0, 0, None, None, 0, C.byref(st), 1, None, None, None) == 0
    assert engine.lib.pisces_hip_vcf_pad_plan(None, 0, 0, None, None, 0, None, 1, None, None, None) == _abi.E_INVALID_ARG
    assert engine.lib.pisces_hip_vcf_pad_plan(None, 1, 0, None, None, 0, C.byref(st), 1, None, None, None) == _abi.E_INVALID_ARG
