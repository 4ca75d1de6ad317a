"""BAM files whose records carry the amplicon name (the XN tag), as data for tests/test_bam_amplicon_cpu.py (no device) and
tests/test_bam_amplicon_gpu.py, and a plain-Python statement of how the reference reads the tag.

Nothing here asks the library: the files are written with tests/bam_synth.BamWriter (raw auxiliary bytes), read back with the plain BAM
reader the BAM tests use, and the expected names come from amplicon_name() below; expected ids are the order in which the names first
appear over the kept reads."""
import functools
import struct

import numpy as np

from tests import bam_synth
from tests.test_bgzf import _bam_reads_reference, _kept

REFS = (("chr1", 1_000_000), ("chr2", 1_000_000))
_SIZE = {ord(c): n for c, n in (("A", 1), ("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4))}


class BadTagType(Exception):
    """TagUtils.GetStringTag's InvalidDataException: the tag's type is neither a string nor a character"""


def amplicon_name(tags):
    """Read.GetAmpliconNameIfExists (Read.cs:483-486) -> BamAlignment.GetStringTagIfTagDataExists("XN") -> TagUtils.GetStringTag
    (BamCommon.cs:1055-1109, 1182-1216) on a record's auxiliary bytes: the FIRST field whose key is XN decides; its type byte is
    upper-cased; Z / H give the bytes up to the NUL, A / C one byte, any other type raises; no such field: None.  The fields in front of
    it are stepped over by their SAM types (specification 4.2.4), B arrays included (the reference's own walk throws on those: the
    deviation the project documents)."""
    p = 0
    while p + 3 <= len(tags):
        key, ty = tags[p:p + 2], tags[p + 2]
        p += 3
        if key == b"XN":
            up = chr(ty).upper()
            if up in "ZH":
                return tags[p:tags.index(b"\0", p)]
            if up in "AC":
                return tags[p:p + 1]
            raise BadTagType(chr(ty))
        if ty in (ord("Z"), ord("H")):
            p = tags.index(b"\0", p) + 1
        elif ty == ord("B"):
            p += 5 + int.from_bytes(tags[p + 1:p + 5], "little") * _SIZE[tags[p]]
        else:
            p += _SIZE[ty]
    return None


def first_appearance_ids(names, known=()):
    """ids by order of first appearance (None -> -1), continuing a dictionary `known` (a list, index = id) -> (ids, dictionary)"""
    table = list(known)
    index = {n: i for i, n in enumerate(table)}
    ids = []
    for n in names:
        if n is None:
            ids.append(-1)
            continue
        if n not in index:
            index[n] = len(table)
            table.append(n)
        ids.append(index[n])
    return np.array(ids, np.int32), table


def read_back(file_bytes, chrom="chr1"):
    """(kept reads of `chrom` by the plain reader, every read of the file)"""
    refs, reads = _bam_reads_reference(file_bytes)
    return _kept(reads, chrom), reads


def xn(name, ty=b"Z"):
    return b"XN" + ty + name + (b"\0" if ty in (b"Z", b"H", b"z", b"h") else b"")


# ---------------------------------------------------------------- case 1: every shape of the tag
NAMES_7 = [b"amp_%03d" % k for k in range(12)]
NAME_40 = [b"panel7/chr1:1000-1400/" + b"%018d" % k for k in range(3)]
NAME_250 = [(b"L%d_" % k) * 100 for k in range(2)]
NAME_250 = [n[:250] for n in NAME_250]
SKIP_KINDS = ("unmapped", "secondary", "duplicate", "mapq0", "other_ref")
OTHER_AUX = b"NMC\x02" + b"MDZ12A3\0" + b"ASi" + struct.pack("<i", 77)
XD = bam_synth.xd_of_runs([(20, "F"), (10, "S"), (20, "R")])
SHAPES = 16


def _shape_record(w, i):
    """Record i of the shapes case: what it is decides i % 16, which name it carries i // 16."""
    kind, j = i % SHAPES, i // SHAPES
    pos, cigar, seq, quals = 1000 + 3 * i, [("M", 50)], "ACGT" * 12 + "AC", [30] * 50
    kw = dict(name=b"r", reverse=bool(i & 1))
    n7 = NAMES_7[j % len(NAMES_7)]
    if kind == 0:
        kw.update(aux=xn(n7) + OTHER_AUX)                                             # first field
    elif kind == 1:
        kw.update(aux=bam_synth.aux_of_every_type() + xn(n7))                        # behind every value type, B arrays among them
    elif kind == 2:
        kw.update(aux=OTHER_AUX + b"XZf" + struct.pack("<f", 1.5) + xn(n7))           # last field
    elif kind == 3:
        kw.update(aux=OTHER_AUX)                                                      # absent
    elif kind == 4:
        kw.update(aux=OTHER_AUX + xn((b"1AE3", b"00FF", b"q")[j % 3], b"H"))          # hex string: its characters are the name
    elif kind == 5:
        kw.update(aux=xn(b"qrs"[j % 3:j % 3 + 1], b"A") + OTHER_AUX)                  # one printable character
    elif kind == 6:
        kw.update(aux=OTHER_AUX + xn(b"tuq"[j % 3:j % 3 + 1], b"c"))                  # int8, read as a character
    elif kind == 7:
        kw.update(aux=xn(b"vwr"[j % 3:j % 3 + 1], b"C"))                              # uint8, read as a character
    elif kind == 8:
        kw.update(aux=xn(n7) + OTHER_AUX + xn(b"second_never_wins"))                  # two XN fields: the first
    elif kind == 9:
        kw.update(aux=b"COZXNZfake\0" + b"XQZabXNAz\0" + (xn(n7) if j & 1 else b""))  # the bytes of a field inside other fields' values
    elif kind == 10:
        kw.update(aux=OTHER_AUX, xd=XD, aux_after=xn(n7))                             # XD in front of XN
    elif kind == 11:
        kw.update(aux=xn(n7), xd=XD, aux_after=OTHER_AUX)                             # XN in front of XD
    elif kind == 12:
        kw.update(aux=xn((b"", b"q", b"")[j % 3]) + OTHER_AUX)                        # the empty name; a one-byte string
    elif kind == 13:
        kw.update(aux=OTHER_AUX + xn(NAME_40[j % 3]))
    elif kind == 14:
        kw.update(aux=xn(NAME_250[j % 2]) + OTHER_AUX)
    else:
        what = SKIP_KINDS[j % len(SKIP_KINDS)]                                        # dropped by ShouldSkipRead: its name is nobody's
        kw.update(aux=xn(b"skipped_" + what.encode()), flag={"unmapped": 0x4, "secondary": 0x100, "duplicate": 0x400}.get(what, 0),
                  mapq=0 if what == "mapq0" else 60, ref_id=1 if what == "other_ref" else 0)
    w.block([pos], cigar, quals, seq=seq, **kw)


@functools.lru_cache(maxsize=None)
def shapes_case(n=704):
    w = bam_synth.BamWriter(REFS)
    for i in range(n):
        _shape_record(w, i)
    return w.finish()


# ---------------------------------------------------------------- one-base reads that carry a name each
def named_file(names, refs=REFS):
    """One kept one-base read per entry of `names` (None: no tag), in that order.  Records that share a name are one block."""
    w = bam_synth.BamWriter(refs)
    where = {}
    for i, n in enumerate(names):
        where.setdefault(n, []).append(i)
    for n, at in where.items():
        w.block(1000 + np.array(at), [("M", 1)], [30], seq="A", name=b"r", aux=b"" if n is None else xn(n), at=at)
    return w.finish()


_ALNUM = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"
# 62 names that differ in their last byte only, eight such families that differ in the byte before: 496 names of one length, so many of
# them meet in one probe chain of a 4 096-slot table, where nothing but their bytes tells them apart
LAST_BYTE = [b"amplicon_with_a_long_common_prefix_" + bytes([f, c]) for f in b"01234567" for c in _ALNUM]
PREFIXES = [b"", b"a", b"am", b"amp", b"amp1", b"amp10", b"amp100", b"amp1000", b"amp10000", b"amp2", b"amp20"]


@functools.lru_cache(maxsize=None)
def probe_case():
    """Names that differ in their last byte only, and names that are prefixes of one another; every name on three reads, the second and
    third round in other orders than the first."""
    pool = LAST_BYTE + PREFIXES
    rng = np.random.default_rng(3)
    names = list(pool) + [pool[k] for k in rng.permutation(len(pool))] + [None] + [pool[k] for k in rng.permutation(len(pool))]
    return names, named_file(names)


N_REGROW = 3000
REGROW_NAMES = [b"n%d" % k for k in range(N_REGROW)]


@functools.lru_cache(maxsize=None)
def regrow_case():
    """3 000 distinct names, more than half of the table's first 4 096 slots, cycled over 6 000 reads: every name recurs"""
    names = REGROW_NAMES + REGROW_NAMES
    return names, named_file(names)


@functools.lru_cache(maxsize=None)
def second_case():
    """Ten names of the regrow case and ten new ones, interleaved, the new ones first"""
    known = [REGROW_NAMES[k] for k in (2999, 0, 17, 1500, 4, 2048, 2047, 999, 1, 2998)]
    fresh = [b"fresh_%d" % k for k in range(10)]
    names = [n for pair in zip(fresh, known) for n in pair] * 2
    return names, named_file(names)


# ---------------------------------------------------------------- refusals: tags that are no string
@functools.lru_cache(maxsize=None)
def bad_type_case():
    """Twelve kept reads: read 5 carries XN:i, read 9 XN:f, the others a proper name"""
    w = bam_synth.BamWriter(REFS)
    for i in range(12):
        aux = b"XNi" + struct.pack("<i", 7) if i == 5 else b"XNf" + struct.pack("<f", 2.5) if i == 9 else xn(b"ok%d" % (i % 3))
        w.block([2000 + i], [("M", 1)], [30], seq="A", aux=aux)
    return w.finish()


# ---------------------------------------------------------------- end to end: the amplicon scenarios as BAM files
def name_of_id(i):
    return None if i < 0 else b"amplicon/%d" % i


def scenario_file(ref, reads, ids):
    """The reads of a scenario of tests/amplicon_cases.py in a BAM, XN = a name per original id, untagged reads untagged"""
    w = bam_synth.BamWriter((("chr1", len(ref)),))
    for r, i in zip(reads, ids):
        w.read(r, aux=b"" if i < 0 else xn(name_of_id(i)))
    return w.finish()
