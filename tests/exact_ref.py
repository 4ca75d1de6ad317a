"""CoverageMethod.Exact, stated once in plain Python: the checker of pisces_hip_exact_span_direction, pisces_hip_get_spanning_read_counts and the
spanning rows of an exact handle.  It shares no code with the library and works the way the reference does, not the way the library does: it
builds the position map and the direction map of a read base by base and scans them (ExactCoverageCalculator.cs), and it keeps the read
summaries in per-position lists inside blocks (RegionStateManager.cs, RegionState.cs).

    Summary                    Read.GetCoverageSummary (Read.cs:83-96, 613-622)
    direction(...)             the per-read decision of CalculateSpanning (ExactCoverageCalculator.cs:62-96), with a trace of the branches taken
    span_of(...)               which allele asks for which span (:18-42)
    ExactState                 AddAlleleCounts' summary bookkeeping (:118-121, 212-219), GetSpanningReadSummaries (:234-254), GetBlock (:361-383),
                               GetCandidatesToProcess' block choice (:295-314) and DoneProcessing (:336-353)
"""
import math
import re

FORWARD, REVERSE, STITCHED = 0, 1, 2
_DIR_KEYS = "FRS"
_CIGAR_RE = re.compile(r"(\d+)([A-Za-z=])")
REF_SPAN = set("MDN=X")     # CigarExtensions.IsReferenceSpan
READ_SPAN = set("MIS=X")    # CigarExtensions.IsReadSpan


class InvalidIndices(Exception):
    """GetDirection's InvalidDataException("Invalid indices -1--1")"""


def parse_cigar(text):
    return [(m.group(2), int(m.group(1))) for m in _CIGAR_RE.finditer(text)]


def parse_directions(text):
    """DirectionInfo(string): "2F:9S:2R" -> [(FORWARD, 2), (STITCHED, 9), (REVERSE, 2)]"""
    return [(_DIR_KEYS.index(tok[-1]), int(tok[:-1])) for tok in text.split(":")]


def runs_of(per_base):
    """Read.GetDirectionInfo: the run-length form of SequencedBaseDirectionMap"""
    runs = []
    for d in per_base:
        if runs and runs[-1][0] == d:
            runs[-1] = (d, runs[-1][1] + 1)
        else:
            runs.append((int(d), 1))
    return runs


def prefix_clip(cigar):
    n = 0
    for op, length in cigar:
        if op == "S":
            n += length
        elif op != "H":
            break
    return n


def suffix_clip(cigar):
    return prefix_clip(list(reversed(cigar)))


class Summary:
    """ReadCoverageSummary: ClipAdjustedStartPosition, ClipAdjustedEndPosition, Cigar, DirectionInfo"""

    def __init__(self, cs, ce, cigar, runs):
        self.cs, self.ce = int(cs), int(ce)
        self.cigar = parse_cigar(cigar) if isinstance(cigar, str) else [(o, int(n)) for o, n in cigar]
        self.runs = parse_directions(runs) if isinstance(runs, str) else [(int(d), int(n)) for d, n in runs]

    @classmethod
    def of_read(cls, position, cigar, per_base_directions):
        """Read.GetCoverageSummary: Position is 1-based, EndPosition = Position + reference span - 1"""
        cigar = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
        ref_span = sum(n for op, n in cigar if op in REF_SPAN)
        end = position + ref_span - 1
        return cls(position - prefix_clip(cigar), end + suffix_clip(cigar), cigar, runs_of(per_base_directions))


def position_map(start, cigar):
    """Read.UpdatePositionMap(position, cigar, map, differentiateSoftClip: true) (Read.cs:564-592)"""
    out, ref = [], start
    for op, length in cigar:
        for _ in range(length):
            if op in READ_SPAN:
                if op in REF_SPAN:
                    out.append(ref)
                    ref += 1
                else:
                    out.append(-2 if op == "S" else -1)
            elif op in REF_SPAN:
                ref += 1
    return out


def direction_map(runs, read_length):
    """Read.UpdateDirectionMap into a new DirectionType[readLength]: entries the runs do not reach keep the array's initial Forward (several
    of the reference's own test summaries are one base short); None when the runs are longer than the read (the reference indexes past the
    end).  A calculator that has seen a read of the same length before finds that read's directions there instead: not modelled, and no
    read's own runs fall short."""
    out = [d for d, n in runs for _ in range(n)]
    return out + [FORWARD] * (read_length - len(out)) if len(out) <= read_length else None


def index_boundaries(start_position, end_position, pmap, trace):
    """GetIndexBoundaries (:162-199)"""
    start_index = end_index = None
    for i, p in enumerate(pmap):
        if 0 <= p <= start_position:
            start_index = i
        if end_index is None and p >= end_position:
            end_index = i
    if start_index is not None and end_index is None and pmap and pmap[-1] == -2:
        trace.append("boundaries:ends-in-soft-clip")
        for i in range(start_index + 1, len(pmap)):
            if pmap[i] == -2:
                end_index = i
                break
    if end_index is not None and start_index is None and pmap and pmap[0] == -2:
        trace.append("boundaries:starts-in-soft-clip")
        for i in range(end_index - 1, -1, -1):
            if pmap[i] == -2:
                start_index = i
                break
    if start_index is None:
        trace.append("boundaries:no-start")
    if end_index is None:
        trace.append("boundaries:no-end")
    if start_index is not None and end_index is not None:
        trace.append("boundaries:both")
    return (-1 if start_index is None else start_index), (-1 if end_index is None else end_index)


def get_direction(preceding_index, trailing_index, dmap, trace):
    """GetDirection (:114-153)"""
    direction = FORWARD
    if preceding_index == -1 and trailing_index == -1:
        trace.append("direction:invalid")
        raise InvalidIndices(f"Invalid indices {preceding_index}-{trailing_index}")
    if trailing_index == preceding_index + 1:
        if preceding_index == -1:
            trace.append("direction:adjacent-no-preceding")
            direction = dmap[trailing_index]
        elif trailing_index == -1:   # (never: it would need precedingIndex == -2)
            trace.append("direction:adjacent-no-trailing")
            direction = dmap[preceding_index]
        else:
            direction = dmap[preceding_index]
            if direction == STITCHED:
                trace.append("direction:adjacent-stitched-takes-trailing")
                direction = dmap[trailing_index]
            else:
                trace.append("direction:adjacent-preceding")
    else:
        if trailing_index == -1:
            trace.append("direction:to-end-of-read")
            trailing_index = len(dmap)
        looped = stopped = False
        for i in range(preceding_index + 1, trailing_index):
            looped = True
            direction = dmap[i]
            if direction == STITCHED:
                stopped = True
                break
        trace.append("direction:between-stops-at-stitched" if stopped else "direction:between-to-the-end" if looped else "direction:between-empty")
    return direction


BRANCHES = ("dropped:outside", "dropped:ends-at-preceding", "dropped:starts-at-trailing", "kept:ends-at-preceding-in-insertion",
            "kept:starts-at-trailing-in-insertion", "one-run",
            "boundaries:ends-in-soft-clip", "boundaries:starts-in-soft-clip", "boundaries:no-start", "boundaries:no-end", "boundaries:both",
            "direction:invalid", "direction:adjacent-no-preceding", "direction:adjacent-stitched-takes-trailing", "direction:adjacent-preceding",
            "direction:to-end-of-read", "direction:between-stops-at-stitched", "direction:between-to-the-end", "direction:between-empty")
# "direction:adjacent-no-trailing" is not among them: trailingIndex == precedingIndex + 1 == -1 needs precedingIndex == -2, which
# GetIndexBoundaries never returns.


def direction(summary, preceding, trailing, trace=None):
    """The body of CalculateSpanning's loop for one summary (:62-96): None when the read is dropped, else the direction it counts in.
    Raises InvalidIndices where the reference throws, ValueError where its maps would not fit the read."""
    trace = [] if trace is None else trace
    cigar = summary.cigar
    first_i = bool(cigar) and cigar[0][0] == "I"     # HasOperationAtOpIndex(0, 'I')
    last_i = bool(cigar) and cigar[-1][0] == "I"     # HasOperationAtOpIndex(0, 'I', fromEnd: true)
    if summary.ce < preceding or summary.cs > trailing:
        trace.append("dropped:outside")
        return None
    if summary.ce == preceding and not last_i:
        trace.append("dropped:ends-at-preceding")
        return None
    if summary.cs == trailing and not first_i:
        trace.append("dropped:starts-at-trailing")
        return None
    if summary.ce == preceding:
        trace.append("kept:ends-at-preceding-in-insertion")
    if summary.cs == trailing:
        trace.append("kept:starts-at-trailing-in-insertion")
    if len(summary.runs) == 1:
        trace.append("one-run")
        return summary.runs[0][0]
    read_length = sum(n for op, n in cigar if op in READ_SPAN)
    dmap = direction_map(summary.runs, read_length)
    if dmap is None:
        raise ValueError("direction runs are longer than the read")
    pmap = position_map(summary.cs - prefix_clip(cigar), cigar)   # (:90) the clip comes off a second time
    pi, ti = index_boundaries(preceding, trailing, pmap, trace)
    return get_direction(pi, ti, dmap, trace)


def span_of(category, position, length):
    """ExactCoverageCalculator.Compute (:18-42): (preceding, trailing); category "insertion" / "deletion" / "mnv" """
    if category == "deletion":
        return position, position + length + 1
    if category == "mnv":
        return position - 1, position + length
    if category == "insertion":
        return position, position + 1
    raise ValueError(category)


class ExactState:
    """The part of RegionStateManager an exact run adds: read summaries by clip-adjusted end inside blocks that come and go."""

    def __init__(self, block_size):
        self.block_size = int(block_size)
        self.blocks = {}          # key -> {position: [Summary]}   (_regionLookup; a block's ReadSummaries by position)
        self.read_length = None   # _readLength: the FIRST read's length
        self.last_up_to_key = None   # _lastUpToBlockKey

    def block_key(self, position):
        return int(math.ceil(position / self.block_size))

    def get_block(self, position, add_if_missing=True):
        if position <= 0:
            raise ValueError("Position must be greater than 0.")
        key = self.block_key(position)
        if key not in self.blocks:
            if not add_if_missing:
                return None
            self.blocks[key] = {}
        return self.blocks[key]

    def add_read(self, position, cigar, per_base_directions):
        """AddAlleleCounts as far as blocks and summaries go: every aligned base and every deleted position touches its block (the tests'
        qualities pass CheckDeletionQuality), then the summary goes into the block of its clip-adjusted end."""
        cigar = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
        if self.read_length is None:
            self.read_length = len(per_base_directions)
        def touch(first, last_position):   # GetBlock for every position first .. last_position
            for k in range(self.block_key(max(first, 1)), self.block_key(last_position) + 1):
                self.blocks.setdefault(k, {})

        ref, last = position, position - 1
        for op, length in cigar:
            if op in REF_SPAN and op in READ_SPAN and length > 0:
                touch(last + 1, ref + length - 1)   # the gap in front of the run, if any (:172-176), and the run
                last = ref + length - 1
            if op in REF_SPAN:
                ref += length
        if (cigar and cigar[-1][0] == "D") or (len(cigar) >= 2 and cigar[-2][0] == "D" and cigar[-1][0] == "S"):
            n = cigar[-1][1] if cigar[-1][0] == "D" else cigar[-2][1]
            touch(last + 1, last + n)   # a deletion at the read's end / in front of its final soft clip (:148-158, :195-210)
        s = Summary.of_read(position, cigar, per_base_directions)
        self.get_block(s.ce).setdefault(s.ce, []).append(s)
        return s

    def spanning_summaries(self, start, end):
        """GetSpanningReadSummaries (:234-254).  The reference's walk starts at `start` itself and GetBlock throws below 1: an MNV at position
        1 asks from 0 and cannot be computed there; the walk here starts at 1."""
        out = []
        if self.read_length is None:
            return out
        for position in range(max(start, 1), end + 2 * self.read_length + 1):
            block = self.get_block(position, False)
            if block is None:
                continue
            out += [s for s in block.get(position, ()) if s.cs <= end and s.ce >= start]
        return out

    def counts(self, preceding, trailing):
        """CalculateSpanning's three counts (EstimatedCoverageByDirection, no redistribution)"""
        out = [0, 0, 0]
        for s in self.spanning_summaries(preceding, trailing):
            d = direction(s, preceding, trailing)
            if d is not None:
                out[d] += 1
        return out

    def compute(self, category, position, length, allele_support):
        cov = self.counts(*span_of(category, position, length))
        total = sum(cov)
        return {"coverage_by_dir": cov, "total_coverage": total, "reference_support": max(0, total - allele_support)}

    def keys_to_flush(self, up_to=None, held_from=None):
        """GetCandidatesToProcess (:295-314): the blocks wholly at or below up_to (all of them when None), ascending, up to the first held one
        (held_from: the lowest key whose MaxAlleleEndpoint reaches past up_to, or None); none at all while up_to stays inside the block
        of the call before (:287-291, :331)"""
        same_block = up_to is not None and self.block_key(up_to) == self.last_up_to_key
        self.last_up_to_key = -1 if up_to is None else self.block_key(up_to)
        if same_block:
            return []
        keys = sorted(k for k in self.blocks if up_to is None or k * self.block_size <= up_to)
        if held_from is not None:
            keys = [k for k in keys if k < held_from]
        return keys

    def done_processing(self, keys):
        for k in keys:
            del self.blocks[k]
