"""Scylla's read pass stated in plain Python, transcribed from the reference's C# (strings and lists, as it builds them) and NOT from
csrc/vead.h: VeadFinder.SetCandidateVariantsFoundInRead / MatchReadVariantsWithVcfVariants / CheckVariantSequenceForMatchInVariantSiteFromRead /
HaveWeSeenEvidenceForAReferenceCall (src/lib/VariantPhasing/Logic/VeadFinder.cs), VcfNeighborhood.SetRangeOfInterest, NeighborhoodReadFilter
and VeadGroupSource.GetVeadGroups.  Positions are Read.Position (1-based), as in PiscesReadBatch.

BRANCHES counts how often each branch of the decision was taken (the fuzz test asserts none of them stayed cold)."""
import collections

NONE, REF, ALT, OTHER = 0, 1, 2, 3
MATCH, INS, DEL = "M", "I", "D"
THIS, INSUFFICIENT, DIFFERENT, REFERENCE, IDONTKNOW = "FoundThisVariant", "HaveInsufficientData", "FoundDifferentVariant", "FoundReferenceVariant", "IDontKnow"

BRANCHES = collections.Counter()


class Site:
    """VariantSite: VcfReferencePosition, VcfReferenceAllele, VcfAlternateAllele"""
    __slots__ = ("pos", "ref", "alt")

    def __init__(self, pos, ref="N", alt="N"):
        self.pos, self.ref, self.alt = pos, ref, alt

    @property
    def has_no_data(self):
        return self.ref == "N" and self.alt == "N"

    @property
    def true_first_base_of_diff(self):
        return self.pos + 1 if len(self.ref) != len(self.alt) else self.pos

    @property
    def type(self):
        if len(self.ref) > len(self.alt):
            return DEL
        if len(self.ref) < len(self.alt):
            return INS
        return MATCH

    def __repr__(self):
        return f"{self.pos}:{self.ref}>{self.alt}"


def segments_of_read(min_q, position, cigar, bases, quals):
    """SetCandidateVariantsFoundInRead: ({type: [Site]}, lastPosInAlignment).  cigar: [(op char, length)]; bases a str."""
    cycle = 0
    ref_position = position - 1          # alignment.Position (0-based)
    found = {DEL: [], MATCH: [], INS: []}
    for op, length in cigar:
        vs = Site(ref_position + 1)
        if op == "S":
            cycle += length
        elif op == "M":
            raw = list(bases[cycle:cycle + length])
            for i in range(length):
                if quals[cycle + i] < min_q:
                    raw[i] = "N"
            vs.ref = "R" * length
            vs.alt = "".join(raw)
            found[MATCH].append(vs)
            cycle += length
            ref_position += length
        elif op == "I":
            ok = quals[cycle] >= min_q
            vs.ref = ""
            vs.alt = bases[cycle:cycle + length]
            if not ok:
                vs.ref = vs.alt = "N"
            vs.pos -= 1
            found[INS].append(vs)
            cycle += length
        elif op == "D":
            if cycle < len(quals):
                after = quals[cycle]
            else:
                after = quals[cycle - 1]
                BRANCHES["deletion quality: after taken from the last base"] += 1
            before = after
            if cycle > 0:
                before = quals[cycle - 1]
            else:
                BRANCHES["deletion quality: before taken from after"] += 1
            ok = before >= min_q and after >= min_q
            vs.alt = ""
            vs.ref = "R" * length
            if not ok:
                vs.ref = vs.alt = "N"
            vs.pos -= 1
            found[DEL].append(vs)
            ref_position += length
        # every other operation: no case in the reference's switch
    return found, ref_position + 1


def check_match(look, query):
    """CheckVariantSequenceForMatchInVariantSiteFromRead"""
    index = look.pos - query.pos
    if index + len(look.alt) > len(query.alt) or index < 0:
        return INSUFFICIENT
    sub = query.alt[index:index + len(look.alt)]
    if sub == look.alt:
        return THIS
    if "N" in sub:
        return INSUFFICIENT
    if sub == look.ref:
        return REFERENCE
    return DIFFERENT


def reference_evidence(look, found):
    """HaveWeSeenEvidenceForAReferenceCall"""
    probe = Site(look.pos, look.ref[:1], look.ref[:1])
    for seg in found[MATCH]:
        if check_match(probe, seg) in (THIS, REFERENCE):
            return True
    return False


def match_sites(sites, found, first, last, min_sites=1):
    """MatchReadVariantsWithVcfVariants: ([state per site], numSitesFoundInRead), or (None, n) when the read is no vead."""
    states = [NONE] * len(sites)
    n_found = 0
    for i, look in enumerate(sites):
        kind = look.type
        if look.true_first_base_of_diff < first or look.true_first_base_of_diff > last:
            BRANCHES["out of range"] += 1
            states[i] = NONE
            continue
        n_found += 1
        if not found[kind]:
            BRANCHES["no segment of the type"] += 1
            states[i] = REF if reference_evidence(look, found) else NONE
            continue
        result = IDONTKNOW
        assigned = None
        for seg in found[kind]:
            if result == THIS:
                break
            if look.pos < seg.pos:
                BRANCHES["gone past"] += 1
                assigned = REF if reference_evidence(look, found) else NONE     # (overwritten below, as in the reference)
                break
            if kind == INS:
                if seg.pos != look.pos:
                    continue
                section = look.alt[1:]
                if seg.has_no_data:
                    result = INSUFFICIENT
                elif seg.alt == section:
                    result = THIS
                else:
                    result = DIFFERENT
            elif kind == DEL:
                if seg.pos != look.pos:
                    continue
                if seg.has_no_data:
                    result = INSUFFICIENT
                elif len(look.ref) - len(look.alt) == len(seg.ref):
                    result = THIS
                else:
                    result = DIFFERENT
            else:
                result = check_match(look, seg)
        del assigned
        if result == IDONTKNOW:
            if reference_evidence(look, found):
                BRANCHES["IDontKnow rescued to reference"] += 1
                result = REFERENCE
        BRANCHES[f"{kind}: {result}"] += 1
        if result in (IDONTKNOW, INSUFFICIENT):
            states[i] = NONE
        elif result == THIS:
            states[i] = ALT
        elif result == DIFFERENT:
            states[i] = OTHER
        else:
            states[i] = REF
    return (states if n_found >= min_sites else None), n_found


def printed(site, state):
    """the VariantSite.ToString() of SetEmptyMatch / SetReferenceMatch / SetVariantMatch / SetDifferenceMatch: the group key's piece"""
    return {NONE: "N>N", REF: f"{site.ref[:1]}>{site.ref[:1]}", ALT: f"{site.ref}>{site.alt}", OTHER: "X>X"}[state]


def canonical(sites, states):
    """equal printed keys <=> equal vectors: the one state of each printed form"""
    out = []
    for s, st in zip(sites, states):
        text = printed(s, st)
        out.append(NONE if text == "N>N" else OTHER if text == "X>X" else REF if text == f"{s.ref[:1]}>{s.ref[:1]}" else ALT)
    return out


def read_states(min_q, position, cigar, bases, quals, sites, min_sites=1):
    """FindVariantResults: (canonical states or None, sites in range, segments)"""
    found, last = segments_of_read(min_q, position, cigar, bases, quals)
    states, n = match_sites(sites, found, position, last, min_sites)
    return (canonical(sites, states) if states is not None else None), n, found


def neighborhood_bounds(sites):
    """SetRangeOfInterest over the sites in the caller's order: (first, last with look-ahead, soft clip end before, soft clip pos after)"""
    last = sites[0].pos
    for vs in sites:
        last = max(last, vs.pos + max(len(vs.alt), len(vs.ref)))
    first = sites[0].pos
    before = first if sites[0].type in (DEL, INS) else first - 1
    after = sites[-1].pos + len(sites[-1].ref)
    return first, last, before, after


def reference_span(cigar):
    return sum(n for op, n in cigar if op in "MDN=X")


def vead_groups(reads, sites, min_q=20, min_sites=1):
    """VeadGroupSource.GetVeadGroups for one neighbourhood.  reads: [(position, cigar, bases, quals)] in file order.
    Returns ([(first read, count, canonical states)] in insertion order, clipped reads, reads used)."""
    first, last, before, after = neighborhood_bounds(sites)
    groups = collections.OrderedDict()
    clipped = used = 0
    for r, (position, cigar, bases, quals) in enumerate(reads):
        end = position + reference_span(cigar) - 1
        starts_s = bool(cigar) and cigar[0][0] == "S"
        ends_s = bool(cigar) and cigar[-1][0] == "S"
        if starts_s and before <= position <= after:
            clipped += 1
        elif ends_s and before <= end <= after:
            clipped += 1
        if end < first:
            continue
        if position > last:
            break
        used += 1
        found, last_pos = segments_of_read(min_q, position, cigar, bases, quals)
        states, _ = match_sites(sites, found, position, last_pos, min_sites)
        if states is None or not states:
            continue
        key = " ".join(printed(s, st) for s, st in zip(sites, states))
        if key not in groups:
            groups[key] = [r, 0, canonical(sites, states)]
        groups[key][1] += 1
    return [tuple(g) for g in groups.values()], clipped, used
