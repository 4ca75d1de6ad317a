"""A vectorised BAM writer that knows what it wrote (SAM/BAM specification sections 4.1 and 4.2).

Records go in as BLOCKS of equal shape (same name length, CIGAR length, sequence length, auxiliary length): one 2-D numpy array a
block, scattered into the stream at the offsets the records' sizes give -- a 34 MB stream of 122 000 records is a few hundred
milliseconds.  A read dict of the form _abi.ReadBatch takes ({pos, cigar, seq, quals, reverse, xd}) is a block of one record.

Beside the bytes the writer keeps what went in, and SynthBam.expected() makes from THAT (never from the bytes) the read batch
pisces_hip_bam_decode must give for a filter: AlignmentSource.ShouldSkipRead (AlignmentsSource.cs:84-92) on the records' flag / mapq /
CIGAR count, the kept records' arrays in file order.  The tests hold the writer to a second opinion by reading its bytes back with the
plain reader of tests/golden/extract_bam_fixture.py."""
import struct
import zlib

import numpy as np

CHUNK = 32768                                   # bam_kernels.hip.h kBamChunk
CIGAR_LETTERS = "MIDNSHP=X"                     # op codes 0-8; 9-15 are reserved and decode to '?'
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"                # SAM specification 4.2.3
DIR_FORWARD, DIR_REVERSE, DIR_STITCHED, DIR_UNTRACKED = 0, 1, 2, 255
_LETTER_OF_OP = np.frombuffer(b"MIDNSHP=X???????", np.uint8)
_LETTER_OF_NIBBLE = np.frombuffer(SEQ_LETTERS.encode(), np.uint8)
_NIBBLE_OF_LETTER = np.full(256, 255, np.uint8)
for _i, _c in enumerate(SEQ_LETTERS):
    _NIBBLE_OF_LETTER[ord(_c)] = _i
_FIXED = np.dtype([("block_size", "<i4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                   ("n_cigar_op", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("next_ref_id", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4")])
assert _FIXED.itemsize == 36


def cigar_words(ops):
    """[(letter or op code, length)] -> uint32 CIGAR words."""
    return np.array([(int(ln) << 4) | (CIGAR_LETTERS.index(op) if isinstance(op, str) else int(op)) for op, ln in ops], np.uint32).reshape(len(ops))


def co_line(n):
    """A header comment line of exactly n >= 5 bytes (to move the first record where a test wants it)."""
    assert n >= 5
    return b"@CO\t" + b"x" * (n - 5) + b"\n"


def xd_of_runs(runs):
    """[(length, 'F' | 'R' | 'S')] -> the Stitcher's XD string."""
    return "".join("%d%s" % (n, d) for n, d in runs)


def aux_of_every_type():
    """Auxiliary fields of every value type of SAM specification 4.2.4 (A c C s S i I f Z H, B with each subtype, an empty Z)."""
    out = b"XAAq" + b"Xcc" + struct.pack("<b", -3) + b"XCC" + struct.pack("<B", 250) + b"Xss" + struct.pack("<h", -300) + b"XSS" + struct.pack("<H", 60000)
    out += b"Xii" + struct.pack("<i", -70000) + b"XII" + struct.pack("<I", 4000000000) + b"Xff" + struct.pack("<f", 1.5)
    out += b"XZZtext\0" + b"XEZ\0" + b"XHH1AE301\0"
    for sub, fmt in ((b"c", "<3b"), (b"C", "<3B"), (b"s", "<3h"), (b"S", "<3H"), (b"i", "<3i"), (b"I", "<3I"), (b"f", "<3f")):
        out += b"XB" + b"B" + sub + struct.pack("<i", 3) + struct.pack(fmt, 1, 2, 3)
    return out + b"X0Bc" + struct.pack("<i", 0)   # (an array of no elements)


def _per_record(v, k, dtype):
    a = np.asarray(v, dtype)
    return np.ascontiguousarray(np.broadcast_to(a, (k,)))


def _rows(v, k, width, dtype):
    a = np.asarray(v, dtype)
    if a.ndim == 1:
        a = a[None, :]
    assert a.shape[1] == width and a.shape[0] in (1, k), (a.shape, k, width)
    return np.ascontiguousarray(np.broadcast_to(a, (k, width)))


class BamWriter:
    def __init__(self, refs=(("chr1", 250_000_000),), header_text=b"@HD\tVN:1.6\n"):
        self.refs = [(n if isinstance(n, str) else n.decode(), int(l)) for n, l in refs]
        self.header = b"BAM\x01" + struct.pack("<i", len(header_text)) + header_text + struct.pack("<i", len(self.refs)) + \
            b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in self.refs)
        self.blocks = []
        self._next = 0
        self.offset = len(self.header)   # where the next record starts, as long as every block is added behind the ones before it

    @staticmethod
    def header_length(refs, l_text):
        return 8 + l_text + 4 + sum(4 + len(n) + 1 + 4 for n, _ in refs)

    def block(self, pos, cigar, quals, seq=None, nibbles=None, packed=None, l_seq=None, ref_id=0, flag=0, reverse=None, mapq=60, name=b"r",
              raw_name=None, aux=b"", xd=None, aux_after=b"", at=None):
        """k = len(pos) records of one shape.
        pos: 1-based positions (the BAM field is pos - 1).  cigar: [(op, len)] for all, or raw uint32 words [n] / [k, n] (any op code).
        seq: letters for all (str / bytes) or [k, l] ASCII; nibbles: 4-bit codes [l] / [k, l]; packed + l_seq: raw packed bytes.
        quals: [l] / [k, l].  ref_id, flag, mapq: one value or [k]; reverse: ORs 0x10 into flag.  name: without its NUL (raw_name: the
        bytes as they are).  aux / aux_after: raw auxiliary bytes in front of / behind the XD:Z field `xd` makes.
        at: the records' indexes in the file (default: behind everything added so far)."""
        pos = np.asarray(pos, np.int64).reshape(-1)
        k = len(pos)
        if isinstance(cigar, list):
            cigar = cigar_words(cigar)
        cigar = np.asarray(cigar, np.uint32)
        cigar = _rows(cigar, k, cigar.shape[-1], np.uint32)
        if packed is not None:
            packed = np.asarray(packed, np.uint8)
            packed = _rows(packed, k, packed.shape[-1], np.uint8)
            assert l_seq is not None and packed.shape[1] == (l_seq + 1) // 2
            nib = np.empty((k, 2 * packed.shape[1]), np.uint8)
            nib[:, 0::2] = packed >> 4
            nib[:, 1::2] = packed & 15
            nibbles = nib[:, :l_seq]
        else:
            if seq is not None:
                letters = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8) if isinstance(seq, (str, bytes, bytearray)) else np.asarray(seq, np.uint8)
                nibbles = _NIBBLE_OF_LETTER[letters]
                assert (nibbles < 16).all(), "a base the 4-bit table cannot express"
            nibbles = np.asarray(nibbles, np.uint8)
            l_seq = nibbles.shape[-1]
            nibbles = _rows(nibbles, k, l_seq, np.uint8)
            padded = np.zeros((k, l_seq + (l_seq & 1)), np.uint8)
            padded[:, :l_seq] = nibbles
            packed = (padded[:, 0::2] << 4) | padded[:, 1::2]
        quals = _rows(np.asarray(quals, np.uint8).reshape(-1, l_seq) if l_seq else np.zeros((1, 0), np.uint8), k, l_seq, np.uint8)
        flag = _per_record(flag, k, np.int64)
        if reverse is not None:
            flag = flag | np.where(_per_record(reverse, k, bool), 0x10, 0)
        name = (bytes(name) + b"\0") if raw_name is None else bytes(raw_name)
        assert len(name) <= 255
        aux_all = bytes(aux) + (b"XDZ" + xd.encode() + b"\0" if xd is not None else b"") + bytes(aux_after)
        if at is None:
            at = np.arange(self._next, self._next + k)
        at = np.asarray(at, np.int64).reshape(-1)
        assert len(at) == k
        self._next = max(self._next, int(at.max()) + 1) if k else self._next
        self.offset += k * (36 + len(name) + 4 * cigar.shape[1] + packed.shape[1] + l_seq + len(aux_all))
        self.blocks.append(dict(k=k, at=at, pos=pos, ref_id=_per_record(ref_id, k, np.int64), flag=flag, mapq=_per_record(mapq, k, np.int64),
                                name=name, cigar=cigar, nibbles=np.ascontiguousarray(nibbles), packed=packed, quals=quals, aux=aux_all, xd=xd, l_seq=l_seq))
        return self

    def filler(self, n_bytes, pos, piece=3000):
        """Plain kept records (1M, one A of quality 30) of n_bytes in all: their size is made with a long Z field."""
        assert n_bytes >= 48
        while n_bytes > 0:
            take = n_bytes if n_bytes <= piece + 48 else piece
            self.block([pos], [("M", 1)], [30], seq="A", name=b"f", aux=b"XFZ" + b"x" * (take - 48) + b"\0")
            n_bytes -= take
        return self

    def read(self, r, **extra):
        """One read dict as _abi.ReadBatch takes it (pos, cigar, seq, quals, reverse, optional xd); extra: any other field of block()."""
        return self.block([r["pos"]], list(r["cigar"]), list(bytes(r["quals"])), seq=r["seq"], reverse=bool(r.get("reverse")), xd=r.get("xd"), **extra)

    def finish(self):
        n = sum(b["k"] for b in self.blocks)
        size = np.zeros(n, np.int64)
        seen = np.zeros(n, np.int64)
        for b in self.blocks:
            b["size"] = 36 + len(b["name"]) + 4 * b["cigar"].shape[1] + b["packed"].shape[1] + b["l_seq"] + len(b["aux"])
            size[b["at"]] = b["size"]
            np.add.at(seen, b["at"], 1)
        assert (seen == 1).all(), "the blocks' `at` must name every record index once"
        at = len(self.header) + np.concatenate([[0], np.cumsum(size)])
        total = int(at[-1])
        assert total < 2 ** 31
        stream = np.zeros(total, np.uint8)
        stream[:len(self.header)] = np.frombuffer(self.header, np.uint8)
        for b in self.blocks:
            k, w = b["k"], b["size"]
            if k == 0:
                continue
            rec = np.empty((k, w), np.uint8)
            fixed = np.zeros(k, _FIXED)
            fixed["block_size"] = w - 4
            fixed["ref_id"] = b["ref_id"]
            fixed["pos"] = b["pos"] - 1
            fixed["l_read_name"] = len(b["name"])
            fixed["mapq"] = b["mapq"]
            fixed["bin"] = 4681
            fixed["n_cigar_op"] = b["cigar"].shape[1]
            fixed["flag"] = b["flag"]
            fixed["l_seq"] = b["l_seq"]
            fixed["next_ref_id"] = -1
            fixed["next_pos"] = -1
            rec[:, :36] = fixed.view(np.uint8).reshape(k, 36)
            p = 36
            for part in (np.frombuffer(b["name"], np.uint8), b["cigar"].astype("<u4").view(np.uint8).reshape(k, 4 * b["cigar"].shape[1]), b["packed"], b["quals"],
                         np.frombuffer(b["aux"], np.uint8)):
                q = p + part.shape[-1]
                rec[:, p:q] = part
                p = q
            assert p == w
            start = at[b["at"]]
            if k == 1 or (np.diff(start) == w).all():       # the block lies in the file as it lies here
                stream[start[0]:start[0] + k * w] = rec.reshape(-1)
            else:
                stream[(start.astype(np.int32)[:, None] + np.arange(w, dtype=np.int32)[None, :]).reshape(-1)] = rec.reshape(-1)
        return SynthBam(self, stream, at[:-1].copy(), size)


class SynthBam:
    def __init__(self, writer, stream, at, size):
        self.refs = writer.refs
        self.blocks = writer.blocks
        self.header_len = len(writer.header)
        self.array = stream                      # the uncompressed stream (uint8)
        self.at = at                             # offset of every record's block_size field, in file order
        self.size = size                         # bytes of every record, block_size field included
        n = len(at)
        self.n_records = n
        self.ref_id, self.flag, self.mapq, self.n_cigar, self.l_seq, self.pos = (np.zeros(n, np.int64) for _ in range(6))
        self.has_xd = np.zeros(n, bool)
        for b in self.blocks:
            i = b["at"]
            self.ref_id[i], self.flag[i], self.mapq[i], self.pos[i] = b["ref_id"], b["flag"], b["mapq"], b["pos"]
            self.n_cigar[i], self.l_seq[i] = b["cigar"].shape[1], b["l_seq"]
            self.has_xd[i] = b["xd"] is not None

    @property
    def stream(self):
        return self.array.tobytes()

    @property
    def n_chunks(self):
        return (len(self.array) + CHUNK - 1) // CHUNK

    def file(self, level=1, member=65280):
        return bgzf(self.array, level, member)

    def keep(self, ref_id, min_map_quality=1, skip_duplicates=True, only_proper_pairs=False):
        """not ShouldSkipRead, for the records of reference sequence ref_id"""
        f = self.flag
        skip = ((f & 0x4) != 0) | ((f & 0x100) != 0) | (bool(only_proper_pairs) & ((f & 0x2) == 0)) | (bool(skip_duplicates) & ((f & 0x400) != 0)) | \
            (self.mapq < min_map_quality) | (self.n_cigar == 0)
        return (self.ref_id == ref_id) & ~skip

    def kept_per_chunk(self, ref_id, **filt):
        """kept reads that START in each 32 KiB chunk of the stream"""
        return np.bincount(self.at[self.keep(ref_id, **filt)] // CHUNK, minlength=self.n_chunks)

    def expected(self, ref_id, min_map_quality=1, skip_duplicates=True, only_proper_pairs=False):
        """The read batch of the kept records, from what went into the writer: dict with the PiscesReadBatch arrays (`arrays`), reads,
        skipped, cigar_ops, bases, index (the kept records' indexes in the file), directions / deletion_directions (None when no kept
        read has an XD tag)."""
        keep = self.keep(ref_id, min_map_quality, skip_duplicates, only_proper_pairs)
        index = np.flatnonzero(keep)
        nr = len(index)
        cig_off = np.concatenate([[0], np.cumsum(np.where(keep, self.n_cigar, 0))])
        seq_off = np.concatenate([[0], np.cumsum(np.where(keep, self.l_seq, 0))])
        no, nb = int(cig_off[-1]), int(seq_off[-1])
        cigar_op, cigar_len = np.zeros(no, np.uint8), np.zeros(no, np.uint32)
        bases, quals = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
        any_xd = bool((keep & self.has_xd).any())
        dirs = np.zeros(nb, np.uint8) if any_xd else None
        ddirs = np.full(2 * no, DIR_UNTRACKED, np.uint8) if any_xd else None
        for b in self.blocks:
            m = keep[b["at"]]
            if not m.any():
                continue
            rows = b["at"][m]
            nc, ls = b["cigar"].shape[1], b["l_seq"]
            words = b["cigar"][m]
            ci = (cig_off[rows][:, None] + np.arange(nc)[None, :]).reshape(-1)
            cigar_op[ci] = _LETTER_OF_OP[words & 15].reshape(-1)
            cigar_len[ci] = (words >> 4).reshape(-1)
            si = (seq_off[rows][:, None] + np.arange(ls)[None, :]).reshape(-1)
            bases[si] = _LETTER_OF_NIBBLE[b["nibbles"][m]].reshape(-1)
            quals[si] = b["quals"][m].reshape(-1)
            if any_xd:
                rev = (b["flag"][m] & 0x10) != 0
                if b["xd"] is None:
                    dirs[si] = np.repeat(np.where(rev, DIR_REVERSE, DIR_FORWARD).astype(np.uint8), ls)
                else:
                    for j in range(len(rows)):
                        d, dd = directions_of(b["xd"], words[j], ls)
                        dirs[seq_off[rows[j]]:seq_off[rows[j]] + ls] = d
                        ddirs[2 * cig_off[rows[j]]:2 * (cig_off[rows[j]] + nc)] = dd
        arrays = dict(position=self.pos[index].astype(np.int32), flags=((self.flag[index] & 0x10) != 0).astype(np.uint8),
                      cigar_offset=np.concatenate([cig_off[:-1][keep], [no]]).astype(np.int32), cigar_op=cigar_op, cigar_len=cigar_len,
                      seq_offset=np.concatenate([seq_off[:-1][keep], [nb]]).astype(np.int32), bases=bases, quals=quals)
        return dict(arrays=arrays, reads=nr, skipped=int((self.ref_id == ref_id).sum()) - nr, cigar_ops=no, bases=nb, index=index,
                    directions=dirs, deletion_directions=ddirs)


def directions_of(xd, words, l_seq):
    """Per-base directions and the (first, last) directions of every deletion, from an XD string's runs over the EXPANDED CIGAR
    (Read.CreateSequencedBaseDirectionMap, Read.cs:664-682; GetDeletionDirectionForStitchedRead, CandidateVariantFinder.cs:468-487);
    what the tag does not reach keeps DirectionType's default (Forward)."""
    ends, kinds, num, end = [], [], "", 0
    for ch in xd:
        if ch.isdigit():
            num += ch
        else:
            end += int(num)
            ends.append(end)
            kinds.append({"F": DIR_FORWARD, "R": DIR_REVERSE, "S": DIR_STITCHED}[ch])
            num = ""
    assert num == ""

    def at(e):
        for x, kd in zip(ends, kinds):
            if e < x:
                return kd
        return DIR_FORWARD
    dirs, dd, e = [], [], 0
    for w in words:
        op, ln = int(w) & 15, int(w) >> 4
        if op in (0, 1, 4, 7, 8):
            dirs += [at(e + j) for j in range(ln)]
        dd += [at(e), at(e + ln - 1)] if op == 2 and ln > 0 else [DIR_UNTRACKED, DIR_UNTRACKED]
        e += ln
    dirs = (dirs + [DIR_FORWARD] * l_seq)[:l_seq]
    return np.array(dirs, np.uint8), np.array(dd, np.uint8)


def bgzf(stream, level=1, member=65280):
    """BGZF members of `member` bytes + the empty end-of-file member (SAM specification 4.1)."""
    data = bytes(stream)
    out = []
    for i in list(range(0, len(data), member)) + [len(data)]:
        chunk = data[i:i + member]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        bsize = 18 + len(payload) + 8
        assert bsize <= 65536
        out.append(b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1) + payload +
                   struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return b"".join(out)


# ---------------------------------------------------------------- the large cases (chunk-count edges of the scans and of the entry kernels)
# (l_seq, CIGAR, name): one to four operations, insertions longer than the 32 bases a candidate record holds inline, deletions, = / X
LARGE_SHAPES = [
    (150, [("M", 150)], b"plain"),
    (36, [("M", 36)], b"s"),
    (151, [("S", 5), ("M", 146)], b"clipped_read"),
    (250, [("M", 100), ("I", 40), ("M", 110)], b"long_insertion"),
    (150, [("M", 70), ("D", 3), ("M", 80)], b"del"),
    (151, [("S", 10), ("=", 60), ("X", 1), ("M", 80)], b"eqx"),
    (250, [("M", 100), ("D", 4), ("M", 148), ("S", 2)], b"del_clip"),
    (36, [("M", 1), ("I", 34), ("M", 1)], b"ins"),
]
LARGE_REFS = (("chr1", 1_000_000), ("chr2", 1_000_000))
# chunk indexes c whose chunks c - 2 and c - 1 hold no kept read at all and whose own first ZERO_KEPT_REACH bytes hold none: the run of
# other records lies across the boundary c - 1 | c, and chunk c still has reads to place (the first chunk of a second workgroup of the
# entry kernels, of a second pass of the scans)
ZERO_KEPT_EDGES = (256, 1024)
ZERO_KEPT_REACH = 8000


def zero_kept_edges(n_chunks):
    return [c for c in ZERO_KEPT_EDGES if c < n_chunks] + ([n_chunks - 1] if n_chunks - 1 < ZERO_KEPT_EDGES[-1] and n_chunks - 1 not in ZERO_KEPT_EDGES else [])


def large_case(n_chunks, seed=0, loci=20_000):
    """A stream of exactly n_chunks 32 KiB chunks of mixed records of chr1 in position order, with runs of chr2 records that cover chunks
    c - 2 and c - 1 whole and reach into chunk c for every c of zero_kept_edges(n_chunks) (ZERO_KEPT_EDGES, and the last chunk of a
    stream that ends in front of the last of them), and a few duplicates
    and mapq-0 records strewn in; reads start every 50 positions over `loci` positions: kept reads, CIGAR operations, bases, candidate slots and pool bytes differ from chunk to chunk."""
    rng = np.random.default_rng(seed)
    sizes = np.array([36 + len(nm) + 1 + 4 * len(cg) + (l + 1) // 2 + l for l, cg, nm in LARGE_SHAPES])
    header_len = BamWriter.header_length(LARGE_REFS, len(b"@HD\tVN:1.6\n"))
    target = n_chunks * CHUNK - 3000 - header_len
    n_max = target // sizes.min() + 1
    # the mix drifts along the file, so that neighbouring chunks differ by more than chance
    drift = np.abs(np.sin(np.arange(n_max) / 900.0))[:, None]
    p = np.array([.3, .1, .15, .1, .1, .1, .1, .05])[None, :] * (1 - drift) + np.array([.05, .4, .05, .05, .05, .05, .05, .3])[None, :] * drift
    shape = (rng.random(n_max)[:, None] > np.cumsum(p / p.sum(1, keepdims=True), 1)).sum(1).clip(0, len(sizes) - 1)
    end = np.cumsum(sizes[shape])
    n = int(np.searchsorted(end, target, side="right"))
    shape, end = shape[:n], end[:n]
    start = header_len + end - sizes[shape]
    ref_id = np.zeros(n, np.int64)
    for c in zero_kept_edges(n_chunks):
        ref_id[(start + sizes[shape] > (c - 2) * CHUNK) & (start < c * CHUNK + ZERO_KEPT_REACH)] = 1
    flag = np.where(rng.random(n) < 0.5, 0x10, 0) | np.where(rng.random(n) < 0.02, 0x400, 0)
    mapq = np.where(rng.random(n) < 0.02, 0, 60)
    # (positions in steps of 50, and one inserted sequence a shape: the reads of a step share their insertions and deletions, which
    # are then frequent enough to be called)
    pos = 500 + (np.arange(n) * (loci / n)).astype(np.int64) // 50 * 50
    w = BamWriter(LARGE_REFS)
    quals_of = np.array([12, 25, 37, 37], np.uint8)
    nibble_of = np.array(([1, 2, 4, 8] * 16)[:63] + [15], np.uint8)
    for s,(l, cg, nm) in enumerate(LARGE_SHAPES):
        i = np.flatnonzero(shape == s)
        # (one random byte a base: six bits choose the base, A C G T with an N once in 64, two bits the quality)
        r = rng.integers(0, 256, (len(i), l), dtype=np.uint8)
        nibbles, at = nibble_of[r & 63], 0
        for op, ln in cg:
            if op == "I":
                nibbles[:, at:at + ln] = np.array([1, 2, 4, 8], np.uint8)[(np.arange(ln) * 7 // 3) % 4]
            at += ln if op in "MIS=X" else 0
        w.block(pos[i], cg, quals_of[r >> 6], nibbles=nibbles, ref_id=ref_id[i], flag=flag[i], mapq=mapq[i], name=nm, at=i)
    bam = w.finish()
    assert bam.n_chunks == n_chunks, (bam.n_chunks, n_chunks)
    return bam
