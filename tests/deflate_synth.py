"""A DEFLATE writer and a tracer for the tests of bgzf_inflate_kernel, written from RFC 1951 / RFC 1952 and the SAM
specification's BGZF section; zlib (the checker of tests/test_bgzf.py) never writes most of what this writes.

  writer   BitWriter, canonical codes from code lengths, tokens Lit / Match, blocks Stored / Fixed / Dynamic with a caller-chosen
           header (code-length code, HCLEN, run-length coding of the lengths).  Everything is asserted (Kraft sums, symbol ranges,
           distance <= bytes so far) unless check=False asks for an illegal stream; Sym and Bits exist only for those.
  members  bgzf_member / build_file lay out BGZF members as make_bgzf of tests/test_bgzf.py does; CRC-32 and ISIZE come from zlib's
           output for the payload (or are given, for the negative table); a subfield in front of 'BC' moves a payload to a chosen
           address residue mod 16.
  tracer   trace(): a plain Python inflate that returns one Event per symbol.  It proves coverage only; expected bytes are zlib's.
  geometry group_offset(): the kernel's bit offset of a symbol inside its group of 64.
  families family_a() ... family_f(): the members of tests/test_deflate_cpu.py and tests/test_deflate_gpu.py."""
import functools
import random
import struct
import zlib
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------- group geometry
LEN_LUT_BITS = 10    # bgzf_kernels.hip.h `#define PISCES_INFLATE_LEN_BITS 10` (kLenLutBits): a longer literal / length code takes the scalar path
DIST_LUT_BITS = 9    # bgzf_kernels.hip.h `#define PISCES_INFLATE_DIST_BITS 9` (kDistLutBits): a longer distance code takes the scalar path


def group_bit(in_offset, bit):
    """bgzf_kernels.hip.h inflate_codes, `const int32_t start = s.in_pos * 8 - s.bitcnt + 8 * skew16`: bits from the 16-byte boundary at or below the payload"""
    return 8 * (in_offset % 16) + bit


def group_offset(in_offset, bit):
    return group_bit(in_offset, bit) % 64


# ---------------------------------------------------------------- RFC 1951 3.2.5 / 3.2.7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
KRAFT_ONE = 1 << 15


class BitWriter:
    """Fields LSB first (RFC 1951 3.1.1); Huffman codes are handed over already bit-reversed, so they go out MSB first."""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n), (value, n)
        self.acc |= value << self.n
        self.n += n
        if self.n >= 64:
            self._flush()

    def _flush(self):
        k = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    def align(self):
        self.bits(0, -self.n % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        self._flush()
        self.buf += data

    def getvalue(self):
        self.align()
        self._flush()
        return bytes(self.buf)


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the codes of one length are consecutive, shorter codes first; returned bit-reversed (None: no code)."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(_reverse(nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    return sum(KRAFT_ONE >> l for l in lengths if l)


def legal_code(lengths, may_be_empty=False):
    """complete, or one single code of one bit (or, for distances, no code at all)"""
    used = [l for l in lengths if l]
    return kraft(lengths) == KRAFT_ONE or used == [1] or (may_be_empty and not used)


def length_symbol(length, alt258=False):
    assert 3 <= length <= 258
    if length == 258:
        return (284, 31, 5) if alt258 else (285, 0, 0)
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def distance_symbol(distance):
    assert 1 <= distance <= 32768
    i = max(k for k in range(30) if DIST_BASE[k] <= distance)
    return i, distance - DIST_BASE[i], DIST_EXTRA[i]


Lit = namedtuple("Lit", "byte")
Match = namedtuple("Match", "length distance alt258", defaults=(False,))
Sym = namedtuple("Sym", "table sym")      # the bare code of a symbol of table 'L' or 'D' (illegal streams only)
Bits = namedtuple("Bits", "value n")      # a raw field (illegal streams only)
Stored = namedtuple("Stored", "data nlen", defaults=(None,))
Fixed = namedtuple("Fixed", "tokens")
Dynamic = namedtuple("Dynamic", "tokens litlen_lengths dist_lengths header eob", defaults=(None, True))
# cl_lengths: the 19 lengths of the code-length code by symbol (None: a balanced code over the symbols used); hclen: 4 ... 19 (None: the
# fewest that hold them); rle: 'none', 'greedy' or an explicit list of (code-length symbol, value of its extra bits)
Header = namedtuple("Header", "cl_lengths hclen rle", defaults=(None, None, "greedy"))


def rle_greedy(seq):
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


def rle_expand(syms):
    out = []
    for s, e in syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + e)
        elif s == 17:
            out += [0] * (3 + e)
        else:
            out += [0] * (11 + e)
    return out


def balanced_lengths(used, n=19):
    syms = sorted(used)
    if len(syms) == 1:   # the code-length code must be complete: a second, unused code
        syms = sorted(syms + [0 if syms[0] else 1])
    k = len(syms)
    d = max(1, (k - 1).bit_length())
    short = (1 << d) - k
    out = [0] * n
    for i, s in enumerate(syms):
        out[s] = d - 1 if i < short else d
    return out


def complete_with_fillers(lengths, fillers):
    """lengths (dict symbol -> bits) made complete: the unused code space goes to symbols of `fillers`, one per power of two."""
    lengths = dict(lengths)
    rest = KRAFT_ONE - sum(KRAFT_ONE >> l for l in lengths.values())
    assert rest >= 0
    fillers = iter([f for f in fillers if f not in lengths])
    for l in range(1, 16):
        if rest & (KRAFT_ONE >> l):
            lengths[next(fillers)] = l
    return lengths


def as_list(lengths, n):
    out = [0] * n
    for s, l in lengths.items():
        out[s] = l
    return out


def write_dynamic_header(w, ll, dl, hdr, check, fields):
    nlen, ndist = len(ll), len(dl)
    if check:
        assert 257 <= nlen <= 286 and 1 <= ndist <= 30 and ll[256]
        assert legal_code(ll) and legal_code(dl, may_be_empty=True), (kraft(ll), kraft(dl))
    fields["hlit"] = w.bitpos
    w.bits(nlen - 257, 5)
    fields["hdist"] = w.bitpos
    w.bits(ndist - 1, 5)
    seq = list(ll) + list(dl)
    syms = [(l, 0) for l in seq] if hdr.rle == "none" else rle_greedy(seq) if hdr.rle == "greedy" else list(hdr.rle)
    if check:
        assert rle_expand(syms) == seq
    used = {s for s, _ in syms}
    cl = list(hdr.cl_lengths) if hdr.cl_lengths is not None else balanced_lengths(used)
    need = max([i + 1 for i in range(19) if cl[CL_ORDER[i]]] + [4])
    hclen = hdr.hclen if hdr.hclen is not None else need
    if check:
        assert kraft(cl) == KRAFT_ONE and max(cl) <= 7 and all(cl[s] for s in used) and need <= hclen and 4 <= hclen <= 19
    fields["hclen"] = w.bitpos
    w.bits(hclen - 4, 4)
    fields["cl"] = []
    for i in range(hclen):
        fields["cl"].append(w.bitpos)
        w.bits(cl[CL_ORDER[i]], 3)
    codes = canonical_codes(cl)
    fields["rle"] = syms
    for s, e in syms:
        if cl[s]:
            w.bits(codes[s], cl[s])
        if s >= 16:
            w.bits(e, {16: 2, 17: 3, 18: 7}[s])
    fields["end"] = w.bitpos


def dynamic_header_bits(ll, dl, hdr=None):
    w = BitWriter()
    write_dynamic_header(w, ll, dl, hdr or Header(), True, {})
    return w.bitpos


class DeflateWriter:
    """One raw DEFLATE stream.  `out` is what the stream decodes to (None once something illegal went in)."""

    def __init__(self, check=True):
        self.w, self.out, self.check, self.blocks, self._cur = BitWriter(), bytearray(), check, [], None

    @property
    def bitpos(self):
        return self.w.bitpos

    def _head(self, final, btype, kind):
        assert self._cur is None
        self.blocks.append({"kind": kind, "header_bit": self.w.bitpos, "fields": {}})
        self.w.bits(int(final), 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535 and (nlen is None or not self.check)
        self._head(final, 0, "stored")
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits(~len(data) & 0xFFFF if nlen is None else nlen, 16)
        self.blocks[-1]["data_byte"] = self.w.bitpos // 8
        self.w.raw(data)
        if self.out is not None:
            self.out += data

    def begin_fixed(self, final=False):
        self._head(final, 1, "fixed")
        self._cur = (FIXED_LL, canonical_codes(FIXED_LL), FIXED_DL, canonical_codes(FIXED_DL))

    def begin_dynamic(self, ll, dl, header=None, final=False):
        self._head(final, 2, "dynamic")
        write_dynamic_header(self.w, ll, dl, header or Header(), self.check, self.blocks[-1]["fields"])
        self._cur = (ll, canonical_codes(ll), dl, canonical_codes(dl))

    def put(self, tokens):
        ll, lc, dl, dc = self._cur
        w, out = self.w, self.out
        for t in tokens:
            if type(t) is Lit:
                assert ll[t.byte]
                w.bits(lc[t.byte], ll[t.byte])
                if out is not None:
                    out.append(t.byte)
            elif type(t) is Match:
                sym, ev, eb = length_symbol(t.length, t.alt258)
                ds, dv, db = distance_symbol(t.distance)
                assert sym < len(ll) and ll[sym] and ds < len(dl) and dl[ds], (sym, ds)
                if ll is FIXED_LL:
                    assert sym < 286 and ds < 30
                w.bits(lc[sym], ll[sym])
                w.bits(ev, eb)
                w.bits(dc[ds], dl[ds])
                w.bits(dv, db)
                if out is not None and t.distance <= len(out):
                    at = len(out) - t.distance
                    if t.distance >= t.length:
                        out += out[at:at + t.length]
                    else:
                        for k in range(t.length):
                            out.append(out[at + k])
                else:
                    assert not self.check, "distance beyond the bytes so far"
                    self.out = out = None
            elif type(t) is Sym:
                assert not self.check
                lens, codes = (ll, lc) if t.table == "L" else (dl, dc)
                w.bits(codes[t.sym], lens[t.sym])
            else:
                assert type(t) is Bits and not self.check
                w.bits(t.value, t.n)

    def end_block(self, eob=True):
        ll, lc = self._cur[:2]
        if eob:
            assert ll[256]
            self.w.bits(lc[256], ll[256])
        self._cur = None

    def block(self, b, final=False):
        if type(b) is Stored:
            self.stored(b.data, final, b.nlen)
        else:
            if type(b) is Fixed:
                self.begin_fixed(final)
            else:
                self.begin_dynamic(b.litlen_lengths, b.dist_lengths, b.header, final)
            self.put(b.tokens)
            self.end_block(b.eob if type(b) is Dynamic else True)

    def payload(self):
        return self.w.getvalue()


def deflate(blocks, check=True):
    w = DeflateWriter(check)
    for i, b in enumerate(blocks):
        w.block(b, final=i == len(blocks) - 1)
    return w


# ---------------------------------------------------------------- BGZF members (RFC 1952 2.3, SAM specification 4.1)
EOF_MEMBER = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 27) + b"\x03\0" + bytes(8)


def zlib_inflate(payload):
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    return out, d.eof


def reference_verdict(payload, isize):
    """What the reference inflater says of a payload with its ISIZE (the CRC aside)."""
    try:
        out, eof = zlib_inflate(payload)
    except zlib.error:
        return False
    return eof and len(out) == isize


class Member:
    """payload: the raw DEFLATE bytes; data: what the builder meant to encode (None for an illegal stream); phase: in_offset % 16 the
    builder asked for (None: wherever the member falls); status: the kInflate* value the negative table expects (None: any nonzero)."""

    def __init__(self, name, payload, data=None, phase=None, isize=None, crc=None, accept=True, status=None, **info):
        self.name, self.payload, self.data, self.phase, self.isize, self.crc = name, payload, data, phase, isize, crc
        self.accept, self.status, self.info, self.in_offset, self.blocks = accept, status, info, None, info.get("blocks")


def member_of(name, blocks, phase=None, check=True, **info):
    w = deflate(blocks, check)
    return Member(name, w.payload(), bytes(w.out) if w.out is not None else None, phase, blocks=w.blocks, **info)


def bgzf_member(payload, isize, crc, pad=0):
    """pad: bytes of a 'PD' subfield in front of 'BC' (0, or 4 and more)"""
    assert pad == 0 or pad >= 4
    extra = (b"PD" + struct.pack("<H", pad - 4) + bytes(pad - 4) if pad else b"") + b"BC" + struct.pack("<H", 2)
    bsize = 12 + len(extra) + 2 + len(payload) + 8
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", len(extra) + 2) + extra + struct.pack("<H", bsize - 1) + payload +
            struct.pack("<II", crc, isize))


BgzfFile = namedtuple("BgzfFile", "data table members")


def build_file(members):
    """The members in order and the end-of-file member; table: (in_offset, in_length, out_offset, out_length, crc32) per block."""
    out, table, total = bytearray(), [], 0
    for m in members:
        pad = 0
        if m.phase is not None:
            e = (m.phase - (len(out) + 18)) % 16
            pad = 0 if e == 0 else e if e >= 4 else e + 16
        isize, crc = m.isize, m.crc
        if isize is None:
            data, eof = zlib_inflate(m.payload)
            assert eof
            isize, crc = len(data), zlib.crc32(data)
        m.in_offset = len(out) + 18 + pad
        assert m.phase is None or m.in_offset % 16 == m.phase
        out += bgzf_member(m.payload, isize, crc if crc is not None else 0, pad)
        table.append((m.in_offset, len(m.payload), total, isize, crc if crc is not None else 0))
        total += isize
    table.append((len(out) + 18, 2, total, 0, 0))
    out += EOF_MEMBER
    return BgzfFile(bytes(out), table, list(members))


# ---------------------------------------------------------------- tracer
Event = namedtuple("Event", "kind code_len bit out_pos sym length distance dist_bit dist_code_len len_extra dist_extra dist_sym block")
Trace = namedtuple("Trace", "out events blocks end_bit")


class TraceError(Exception):
    pass


def _decoder(lengths):
    codes = canonical_codes(lengths)
    table = {(l << 16) | c: s for s, (l, c) in enumerate(zip(lengths, codes)) if l}
    return table, sorted({l for l in lengths if l})


def trace(payload, in_offset=0):
    """Inflate `payload` one symbol at a time.  Events: kind 'literal' / 'length' / 'eob' (code_len, bit of the code's first bit,
    out_pos; for 'length' also length, distance, where the distance code starts and how long it is, extra-bit counts) and 'stored'
    (bit = first bit of the data, length = LEN).  blocks: kind, header_bit, and for dynamic blocks the header's numbers."""
    n_bits = 8 * len(payload)
    padded = payload + bytes(8)
    pos = 0

    def peek(p, n):
        if p + n > n_bits + 64:
            raise TraceError("out of input")
        return (int.from_bytes(padded[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)

    def take(n):
        nonlocal pos
        v = peek(pos, n)
        pos += n
        return v

    def decode(dec):
        nonlocal pos
        table, lens = dec
        v = peek(pos, 15) if pos + 15 <= n_bits + 64 else 0
        for l in lens:
            s = table.get((l << 16) | (v & ((1 << l) - 1)))
            if s is not None:
                pos += l
                return s, l
        raise TraceError("no code")

    out, events, blocks = bytearray(), [], []
    while True:
        blk = {"header_bit": pos}
        final, btype = take(1), take(2)
        bi = len(blocks)
        blocks.append(blk)
        if btype == 0:
            blk["kind"] = "stored"
            pos += -pos % 8
            n, nn = take(16), take(16)
            if n != (~nn & 0xFFFF) or pos + 8 * n > n_bits:
                raise TraceError("stored")
            events.append(Event("stored", 0, pos, len(out), None, n, None, None, None, None, None, None, bi))
            out += payload[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        elif btype in (1, 2):
            if btype == 1:
                blk["kind"] = "fixed"
                ll, dl = FIXED_LL, FIXED_DL
            else:
                blk["kind"] = "dynamic"
                nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[CL_ORDER[i]] = take(3)
                if nlen > 286 or ndist > 30 or kraft(cl) != KRAFT_ONE:
                    raise TraceError("header")
                dec, seq, rle = _decoder(cl), [], []
                while len(seq) < nlen + ndist:
                    s, _ = decode(dec)
                    if s < 16:
                        seq.append(s)
                        continue
                    if s == 16 and not seq:
                        raise TraceError("repeat")
                    rep = 3 + take(2) if s == 16 else 3 + take(3) if s == 17 else 11 + take(7)
                    rle.append((s, rep, len(seq)))
                    seq += [seq[-1] if s == 16 else 0] * rep
                if len(seq) > nlen + ndist:
                    raise TraceError("repeat")
                ll, dl = seq[:nlen], seq[nlen:]
                if not ll[256] or not legal_code(ll) or not legal_code(dl, True):
                    raise TraceError("lengths")
                blk.update(nlen=nlen, ndist=ndist, ncode=ncode, rle=rle, cl=cl)
            blk.update(n_ll=sum(1 for l in ll if l), n_dl=sum(1 for l in dl if l), max_ll=max(ll), max_dl=max(dl))
            ldec, ddec = _decoder(ll), _decoder(dl)
            while True:
                at = pos
                s, cl_ = decode(ldec)
                if s < 256:
                    events.append(Event("literal", cl_, at, len(out), s, None, None, None, None, None, None, None, bi))
                    out.append(s)
                elif s == 256:
                    events.append(Event("eob", cl_, at, len(out), s, None, None, None, None, None, None, None, bi))
                    break
                else:
                    if s > 285:
                        raise TraceError("length symbol")
                    eb = LEN_EXTRA[s - 257]
                    length = LEN_BASE[s - 257] + take(eb)
                    dat = pos
                    ds, dcl = decode(ddec)
                    if ds > 29:
                        raise TraceError("distance symbol")
                    deb = DIST_EXTRA[ds]
                    dist = DIST_BASE[ds] + take(deb)
                    if dist > len(out):
                        raise TraceError("too far")
                    events.append(Event("length", cl_, at, len(out), s, length, dist, dat, dcl, eb, deb, ds, bi))
                    for k in range(length):
                        out.append(out[-dist])
        else:
            raise TraceError("block type")
        if final:
            break
    if pos > n_bits:
        raise TraceError("out of input")
    return Trace(bytes(out), events, blocks, pos)


# ---------------------------------------------------------------- family A: every construct at every group offset
A_PREAMBLE = 24600   # bytes of history in front: distance symbols 28 and 29 (13 extra bits) start at 16385 and 24577
A_LITS = {"lit2": 0x41, "lit3": 0x42, "lit9": 0x43, "lit10": 0x44, "lit11": 0x45, "lit15": 0x46}
# (length-code bits, extra bits) of the four length constructs; (distance-code bits, extra bits) of the eight distance constructs
A_LENGTHS = ((4, 0), (10, 5), (11, 0), (15, 5))
A_DISTANCES = tuple((b, e) for b in (8, 9, 10, 15) for e in (0, 13))
A_EOB = (4, 12)


def _a_codes(eob_bits, which):
    ll = {0x41: 2, 0x42: 3, 257: 4, 256: eob_bits, 0x43: 9, 0x44: 10, 0x45: 11, 0x46: 15, 281: 10, 258: 11, 282: 15}
    ll = as_list(complete_with_fillers(ll, range(0x80, 0x100)), 286)
    dl = ({0: 8, 1: 9, 2: 10, 3: 15, 28: 8, 29: 9}, {0: 10, 1: 15, 2: 8, 3: 9, 28: 10, 29: 15})[which]
    dl = as_list(complete_with_fillers(dl, range(4, 28)), 30)
    return ll, dl


@functools.lru_cache(None)
def family_a():
    """Two dynamic codes (a short and a long end-of-block code; between them every distance-code length with 0 and with 13 extra bits),
    each in two members of 32 blocks.  Block i is padded with 2- and 3-bit literals so that its token sequence starts at group offset i:
    the sequence is the same in every block, so each of its constructs walks through all 64 offsets."""
    rng = np.random.default_rng(101)
    pre = rng.integers(0, 256, A_PREAMBLE, dtype=np.uint8).tobytes()
    members = []
    for which, eob_bits in enumerate(A_EOB):
        ll, dl = _a_codes(eob_bits, which)
        hbits = 3 + dynamic_header_bits(ll, dl)
        for half in range(2):
            phase = (3, 8, 13, 0)[2 * which + half]
            w = DeflateWriter()
            w.stored(pre)
            for i in range(32 * half, 32 * half + 32):
                pad = (i - group_offset(phase, w.bitpos + hbits)) % 64
                pad += 64 if pad == 1 else 0
                w.begin_dynamic(ll, dl, final=i % 32 == 31)
                w.put([Lit(0x42)] * (pad % 2) + [Lit(0x41)] * ((pad - 3 * (pad % 2)) // 2))
                assert group_offset(phase, w.bitpos) == i
                w.put([Lit(b) for b in A_LITS.values()])
                x5 = 31 * (i % 2)
                far = lambda base: base + (min(8191, len(w.out) - base) if i % 2 else 0)
                for length, dist in ((3, 1), (3, 16385), (131 + x5, 2), (131 + x5, 24577), (4, 3), (4, 16385), (163 + x5, 4), (163 + x5, 24577)):
                    w.put([Match(length, far(dist) if dist > 4 else dist)])
                w.end_block()
            members.append(Member(f"A/eob{eob_bits}/blocks{32 * half}-{32 * half + 31}", w.payload(), bytes(w.out), phase, blocks=w.blocks))
    return build_file(members)


# ---------------------------------------------------------------- family B: code shapes
SMALL_LL = as_list({0x61: 2, 0x62: 3, 0x63: 3, 0x64: 3, 256: 3, 257: 3, 258: 3}, 259)
SMALL_DL = [2, 2, 3, 3, 3, 3]
EOB_ONLY_LL = [0] * 256 + [1]
SMALL_TOKENS = [Lit(0x61), Lit(0x62), Lit(0x63), Match(3, 1), Lit(0x64), Match(4, 2), Match(3, 3)]
ALL_LL = [8] * 226 + [9] * 60    # 286 symbols, complete
ALL_DL = [4] * 2 + [5] * 28      # 30 symbols, complete


def all_symbol_tokens():
    """Every length symbol and every distance symbol at the lowest and the highest value of its extra bits (32 768 bytes in front)."""
    lens = []
    for i in range(29):
        lens += [(LEN_BASE[i], False), (LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1, False)]
    lens[-1] = (258, True)   # symbol 284 with extra bits 31 beside symbol 285
    dists = []
    for i in range(30):
        dists += [DIST_BASE[i], DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1]
    toks = [Lit(0x41), Lit(0xF0)]
    for k in range(max(len(lens), len(dists))):
        l, alt = lens[k % len(lens)]
        toks.append(Match(l, dists[k % len(dists)], alt))
    return toks


@functools.lru_cache(None)
def family_b():
    rng = np.random.default_rng(102)
    m = []
    ll1 = as_list({0x61: 1, 256: 2, 257: 3, 264: 3}, 265)
    m.append(member_of("B/single_distance_code", [Dynamic([Lit(0x61), Match(3, 1), Match(10, 1), Lit(0x61)], ll1, [1])]))
    m.append(member_of("B/single_distance_code_symbol4", [Dynamic([Lit(0x61)] * 6 + [Match(3, 5), Match(10, 6)], ll1, [0, 0, 0, 0, 1])]))
    empty = Dynamic([], EOB_ONLY_LL, [0])
    data = Fixed([Lit(0x41), Lit(0x42), Match(5, 2)])
    small = Dynamic(SMALL_TOKENS, SMALL_LL, SMALL_DL)
    m.append(member_of("B/eob_only_first", [empty, data, small]))
    m.append(member_of("B/eob_only_middle", [data, empty, small]))
    m.append(member_of("B/eob_only_last", [data, small, empty]))
    m.append(member_of("B/eob_only_alone", [empty]))
    m.append(member_of("B/no_distance_code", [Dynamic([Lit(0x61), Lit(0x62), Lit(0x61), Lit(0x64)], SMALL_LL, [0])]))
    # minima: HLIT 257, HDIST 1; HCLEN 4 holds only 16 / 17 / 18 / 0, which cannot announce an end-of-block code, so the smallest
    # legal HCLEN is 5 (symbol 8: 256 codes of 8 bits); HCLEN 4 itself is a row of the negative table
    ll_min = [8] * 255 + [0, 8]
    m.append(member_of("B/minimal_header", [Dynamic([Lit(0), Lit(7), Lit(254)], ll_min, [0], Header(as_list({8: 1, 0: 1}, 19), 5, "none"))]))
    m.append(member_of("B/maximal_header", [Dynamic(all_symbol_tokens()[:2] + [Match(258, 1), Match(3, 2), Lit(0x41)], ALL_LL, ALL_DL,
                                                    Header(as_list({8: 1, 9: 2, 4: 3, 5: 4, 0: 5, 16: 6, 17: 7, 15: 7}, 19), 19, "greedy"))]))
    # repeat codes
    ll16 = [8] * 255 + [0, 8]   # 255 literals and the end-of-block code, 8 bits each
    m.append(member_of("B/repeat16_after_first_length", [Dynamic([Lit(1), Lit(2)], ll16, [0],
                       Header(rle=[(8, 0)] + [(16, 3)] * 41 + [(16, 2), (16, 0), (0, 0), (8, 0), (0, 0)]))]))
    ll_cross = as_list({0x61: 1, 256: 2, 257: 3, 258: 3}, 259)   # the length of symbol 257 (3 bits) is repeated over symbol 258 and four distance lengths
    m.append(member_of("B/repeat16_into_distance_lengths", [Dynamic([Lit(0x61), Match(3, 1), Match(4, 2)], ll_cross, [3, 3, 3, 3, 2, 2],
                       Header(rle=rle_greedy(ll_cross[:258]) + [(16, 2), (2, 0), (2, 0)]))]))
    # 17 with 3 and with 10 zeros, 18 with 11 and with 138, the last run ending exactly on nlen + ndist
    ll_runs = [0] * 286
    for s, l in {0: 2, 4: 2, 15: 3, 27: 3, 166: 4, 256: 4, 285: 3}.items():   # zero runs of 3 (1-3), 10 (5-14), 11 (16-26), 138 (28-165)
        ll_runs[s] = l
    assert kraft(ll_runs) == KRAFT_ONE
    dl_runs = [1, 1] + [0] * 28
    hdr = Header(rle=[(2, 0), (17, 0), (2, 0), (17, 7), (3, 0), (18, 0), (3, 0), (18, 127), (4, 0), (18, 78), (4, 0), (18, 17), (3, 0), (1, 0), (1, 0), (18, 17)])
    m.append(member_of("B/repeat17_18_extremes_and_exact_end", [Dynamic([Lit(0), Lit(4), Lit(15), Lit(27), Lit(166), Match(258, 1), Match(258, 2)], ll_runs, dl_runs, hdr)]))
    # 15-bit-deep codes of both kinds in one block
    deep_ll = as_list(complete_with_fillers({0x61: 15, 0x62: 15, 256: 14, 257: 13, 285: 15}, [c for c in range(0x30, 0x60)]), 286)
    deep_dl = as_list(complete_with_fillers({0: 15, 1: 15, 2: 14}, range(3, 30)), 30)
    m.append(member_of("B/deep_codes", [Dynamic([Lit(0x61), Lit(0x62), Match(3, 1), Match(258, 2), Match(3, 3), Lit(0x61)] * 9, deep_ll, deep_dl)]))
    # every length and distance symbol, behind 32 KiB of history
    noise = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    m.append(member_of("B/all_symbols_dynamic", [Stored(noise), Dynamic(all_symbol_tokens(), ALL_LL, ALL_DL)]))
    m.append(member_of("B/all_symbols_fixed", [Stored(noise), Fixed(all_symbol_tokens())]))
    return build_file(m)


# ---------------------------------------------------------------- family C: block transitions
def _c_block(kind, k, first):
    """A small block of `kind`; k shifts where it ends: k nine-bit literals in a fixed block, k three-bit literals in a dynamic one."""
    if kind == "stored":
        return Stored(b"stored" + bytes([48 + k]))
    if kind == "fixed":
        return Fixed([Lit(0x41), Lit(0x42)] + [Lit(0xF0 + k)] * k + ([] if first else [Match(4, 3)]))
    return Dynamic([Lit(0x61), Lit(0x62)] + [Lit(0x63)] * k + ([] if first else [Match(4, 3)]), SMALL_LL, SMALL_DL)


C_STORED_SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65)
C_LARGEST_STORED = 65536 - 26 - 5   # a member is at most 64 KiB: 18 + 8 bytes of header and trailer, 5 of the stored block's own
C_TRAILING = (1, 7, 8, 9, 40)


@functools.lru_cache(None)
def family_c():
    rng = np.random.default_rng(103)
    kinds = ("stored", "fixed", "dynamic")
    m = []
    for a in kinds:
        for b in kinds:
            for k in range(8):
                m.append(member_of(f"C/pair/{a}-{b}/{k}", [_c_block(a, k, True), _c_block(b, 0, False)], pair=(a, b)))
    for r in range(16):
        for n in C_STORED_SIZES:
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            m.append(member_of(f"C/stored/residue{r}/size{n}", [Stored(data), Fixed([Lit(0x41), Lit(0x42), Match(3, 2)]), Stored(b"xyz")], phase=(r - 5) % 16))
    m.append(member_of("C/stored/largest", [Stored(rng.integers(0, 256, C_LARGEST_STORED, dtype=np.uint8).tobytes())]))
    tail = Fixed([Lit(0x41), Lit(0x42), Match(6, 2)])
    m.append(member_of("C/empty200/stored", [Stored(b"")] * 200 + [tail]))
    m.append(member_of("C/empty200/fixed", [Fixed([])] * 200 + [tail]))
    m.append(member_of("C/empty200/dynamic", [Dynamic([], SMALL_LL, SMALL_DL)] * 200 + [tail]))
    m.append(member_of("C/empty200/dynamic_eob_only", [Dynamic([], EOB_ONLY_LL, [0])] * 200 + [tail]))
    for a in kinds:
        first = {"stored": Stored(b"abcdefg"), "fixed": Fixed([Lit(c) for c in b"abcdefg"]),
                 "dynamic": Dynamic([Lit(0x61), Lit(0x62), Lit(0x63), Lit(0x64), Lit(0x61), Lit(0x62), Lit(0x63)], SMALL_LL, SMALL_DL)}[a]
        for b in kinds[1:]:
            for back in (7, 6):
                toks = [Match(4, back), Lit(0x61), Match(3, 3)]
                m.append(member_of(f"C/reach_back/{a}-{b}/distance{back}", [first, Fixed(toks) if b == "fixed" else Dynamic(toks, SMALL_LL, SMALL_DL)],
                                   reach=(a, b, back)))
    for k in range(8):   # 3 + 16 + 9 k + 7 bits: the end-of-block code ends 0 ... 7 bits before the payload does
        m.append(member_of(f"C/final_eob/{k}", [Fixed([Lit(0x41), Lit(0x42)] + [Lit(0xF0)] * k)]))
    for n in C_TRAILING:
        base = member_of("", [Fixed([Lit(0x41), Lit(0x42), Match(9, 2)])])
        m.append(Member(f"C/trailing/{n}", base.payload + rng.integers(1, 256, n, dtype=np.uint8).tobytes(), base.data, trailing=n))
    return build_file(m)


# ---------------------------------------------------------------- family D: what one group writes
# Only codes of at most 10 (literal / length) and 9 (distance) bits: no symbol of these members stops the walk except the end-of-block
# code, so a group's literals and pairs are written by ONE call of the kernel's emit() and the sizes below are what that call sees.
D_LL = as_list({0x41: 1, 0x42: 3, 256: 4, 257: 4, 258: 4, 285: 4, 261: 6, 264: 6, 265: 6, 269: 6, 273: 6, 277: 6, 281: 6, 0x43: 6}, 286)
D_DL = ALL_DL
P_LL = as_list({257: 1, 0x42: 2, 256: 2}, 258)
P_DL = [1, 1]
assert kraft(D_LL) == KRAFT_ONE and kraft(P_LL) == KRAFT_ONE


def _d_claim(tokens):
    """pairs, their bytes, and how far the furthest source reaches past the group's first output byte (<= 0: not at all)"""
    at, pairs, nbytes, reach = 0, 0, 0, None
    for t in tokens:
        if type(t) is Match:
            pairs += 1
            nbytes += t.length
            reach = max(at - t.distance + t.length, reach if reach is not None else -1 << 30)
            at += t.length
        else:
            at += 1
    return dict(pairs=pairs, pair_bytes=nbytes, reach=reach)


D_SHAPES = [
    ("lit64", [Lit(0x41)] * 64, dict(lits=64)),
    ("pair_bytes63", [Match(42, 200), Match(21, 200)], {}),
    ("pair_bytes64", [Match(42, 200), Match(22, 200)], {}),
    ("pair_bytes65", [Match(42, 200), Match(19, 200), Match(4, 200)], {}),
    ("source_ends_at_group_start", [Match(10, 10)], {}),
    ("source_ends_one_past_group_start", [Match(10, 9)], {}),
    ("source_ends_at_group_start_behind_literals", [Lit(0x42), Lit(0x42), Match(10, 12)], {}),
    ("source_ends_one_past_behind_literals", [Lit(0x42), Lit(0x42), Match(10, 11)], {}),
    ("source_is_literal_of_the_group", [Lit(0x42), Lit(0x43), Lit(0x42), Match(3, 3)], {}),
    ("two_overlapping_pairs", [Match(10, 2), Match(10, 5)], {}),
] + [(f"overlap258_distance{d}", [Match(258, d)], {}) for d in (1, 2, 3, 63, 64, 65, 100, 258, 259)]


@functools.lru_cache(None)
def family_d():
    rng = np.random.default_rng(104)
    pre = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    m = []
    for name, toks, extra in D_SHAPES:
        for ends in (False, True):   # ends: the member's output ends inside the group (ISIZE reached there)
            if name == "lit64" and ends:
                toks, extra = toks[:60], dict(lits=60)
            phase = len(m) % 16
            w = DeflateWriter()
            w.stored(pre)
            w.begin_dynamic(D_LL, D_DL, final=True)
            w.put([Lit(0x42)])
            while group_offset(phase, w.bitpos):
                w.put([Lit(0x41)])
            claim = dict(_d_claim(toks), bit=w.bitpos, **extra)
            w.put(toks)
            if not ends:
                w.put([Lit(0x41)] * 70)
            w.end_block()
            m.append(Member(f"D/{name}" + ("/ends_in_group" if ends else ""), w.payload(), bytes(w.out), phase, claim=claim, blocks=w.blocks))
    for ends in (False, True):   # 32 two-bit pairs; the header's length (HCLEN) is what makes the two-bit steps meet offset 0
        for hclen in range(4, 20):
            phase = len(m) % 16
            w = DeflateWriter()
            w.stored(pre)
            try:
                w.begin_dynamic(P_LL, P_DL, Header(hclen=hclen), final=True)
            except AssertionError:
                continue
            w.put([Lit(0x42)])
            if group_offset(phase, w.bitpos) % 2:
                continue
            while group_offset(phase, w.bitpos):
                w.put([Lit(0x42)])
            toks = [Match(3, 1)] * (30 if ends else 32)
            claim = dict(_d_claim(toks), bit=w.bitpos, lits=0)
            w.put(toks + ([] if ends else [Lit(0x42)] * 40))
            w.end_block()
            m.append(Member("D/pairs32" + ("/ends_in_group" if ends else ""), w.payload(), bytes(w.out), phase, claim=claim, blocks=w.blocks))
            break
        else:
            raise AssertionError("no header length aligns the pairs")
    return build_file(m)


# ---------------------------------------------------------------- family E: the negative table
def _bad(name, blocks, isize, status, **kw):
    w = deflate(blocks, check=False)
    return Member(name, w.payload(), None, None, isize, 0, accept=False, status=status, blocks=w.blocks, **kw)


@functools.lru_cache(None)
def family_e():
    """Rows: payload, ISIZE, the status of bgzf_kernels.hip.h's enum (None: any nonzero).  The reference rejects every one of them."""
    L = lambda s: [Lit(c) for c in s]
    rows = []
    good = deflate([Fixed(L(b"truncated payload: the stream runs on into the trailer") * 3)])
    rows.append(Member("E/truncated", good.payload()[:40], None, None, len(good.out), 0, accept=False, status=None))
    rows.append(Member("E/block_type_3", bytes([0x07]), None, None, 0, 0, accept=False, status=2))
    rows.append(_bad("E/stored_nlen_mismatch", [Stored(b"abcd", nlen=0x1234)], 4, 3))
    ok_ll, ok_dl = SMALL_LL, SMALL_DL
    body = [Lit(0x61)]
    rows.append(_bad("E/lengths/litlen_oversubscribed", [Dynamic(body, as_list({0x61: 1, 0x62: 1, 256: 1}, 257), [1], eob=False)], 1, 4))
    rows.append(_bad("E/lengths/distance_oversubscribed", [Dynamic(body, ok_ll, [1, 1, 1], eob=False)], 1, 4))
    rows.append(_bad("E/lengths/code_length_code_oversubscribed", [Dynamic(body, ok_ll, ok_dl, Header(as_list({0: 1, 2: 1, 3: 1, 1: 2}, 19)), eob=False)], 1, 4))
    rows.append(_bad("E/lengths/litlen_incomplete", [Dynamic(body, as_list({0x61: 2, 256: 2}, 257), [1], eob=False)], 1, 4))
    rows.append(_bad("E/lengths/distance_incomplete", [Dynamic(body, ok_ll, [2, 2], eob=False)], 1, 4))
    rows.append(_bad("E/lengths/code_length_code_incomplete", [Dynamic(body, ok_ll, ok_dl, Header(as_list({0: 2, 2: 2, 3: 2, 1: 3}, 19)), eob=False)], 1, 4))
    rows.append(_bad("E/lengths/no_end_of_block_code_hclen4", [Dynamic([], [0] * 257, [0], Header(as_list({18: 1, 0: 1}, 19), 4, [(18, 127), (18, 109)]), eob=False)], 0, 4))
    rows.append(_bad("E/lengths/no_end_of_block_code", [Dynamic(body, as_list({0x61: 1, 0x62: 1}, 257), [1], eob=False)], 1, 4))
    rows.append(_bad("E/lengths/repeat16_first", [Dynamic([], ok_ll, ok_dl, Header(as_list({16: 1, 0: 2, 2: 3, 3: 3}, 19), rle=[(16, 0)] + rle_greedy(ok_ll + ok_dl)[1:]), eob=False)], 0, 4))
    rows.append(_bad("E/lengths/repeat_past_the_end", [Dynamic([], ok_ll, ok_dl, Header(rle=rle_greedy(ok_ll + ok_dl)[:-3] + [(18, 0)]), eob=False)], 0, 4))
    for nlen in (287, 288):
        rows.append(_bad(f"E/lengths/hlit{nlen - 257}", [Dynamic([], [8] * 144 + [9] * 112 + [7] * 24 + [8] * (nlen - 280), [5] * 30, eob=False)], 0, 4))
    for ndist in (31, 32):
        rows.append(_bad(f"E/lengths/hdist{ndist - 1}", [Dynamic([], ALL_LL, [5] * ndist, eob=False)], 0, 4))
    for s in (286, 287):
        rows.append(_bad(f"E/symbol/fixed_litlen_{s}", [Fixed(L(b"ab") + [Sym("L", s)])], 2, 5))
    for s in (30, 31):
        rows.append(_bad(f"E/symbol/fixed_distance_{s}", [Fixed(L(b"ab") + [Sym("L", 257), Sym("D", s)])], 5, 5))
    ll1 = as_list({0x61: 1, 256: 2, 257: 3, 264: 3}, 265)
    rows.append(_bad("E/symbol/single_distance_code_unused_pattern", [Dynamic([Lit(0x61), Sym("L", 257), Bits(1, 1)], ll1, [1])], 4, 5))
    rows.append(_bad("E/symbol/single_litlen_code_unused_pattern", [Dynamic([Bits(1, 1)], EOB_ONLY_LL, [0], eob=False)], 0, 5))
    rows.append(_bad("E/symbol/length_without_distance_codes", [Dynamic([Lit(0x61), Sym("L", 257), Bits(0, 5)], ll1, [0])], 4, 5))
    rows.append(_bad("E/symbol/fifteen_bits_without_a_code", [Dynamic([Lit(0x61), Sym("L", 257), Bits(0x7FFF, 15)], ll1, [1])], 4, 5))
    rows.append(_bad("E/distance/at_output_start", [Fixed([Match(3, 1)])], 3, 6))
    rows.append(_bad("E/distance/after_stored_block", [Stored(b"abcde"), Fixed([Match(3, 6)])], 8, 6))
    rows.append(_bad("E/distance/behind_literals_of_the_group", [Fixed(L(b"abc") + [Match(3, 4)])], 6, 6))
    deep = as_list(complete_with_fillers({0x61: 1, 0x62: 11, 256: 2}, range(0x30, 0x60)), 257)
    over = {"literal": [Fixed(L(b"abcde"))], "pair": [Fixed(L(b"ab") + [Match(3, 2)])], "stored": [Stored(b"abcde")],
            "long_coded_literal": [Dynamic(L(b"aaaa") + [Lit(0x62)], deep, [0])]}
    for how, blocks in over.items():
        rows.append(_bad(f"E/overflow/{how}", blocks, 4, 7))
    rows.append(_bad("E/short/one_byte_missing", [Fixed(L(b"abcde"))], 6, 8))
    return rows


def negative_file(row):
    """The bad member between two valid ones: it is block 1."""
    good = [member_of("before", [Fixed([Lit(c) for c in b"before"])]), member_of("after", [Dynamic(SMALL_TOKENS, SMALL_LL, SMALL_DL)])]
    return build_file([good[0], row, good[1]])


# ---------------------------------------------------------------- family F: grammar fuzz
def random_complete_lengths(rng, k, maxbits=15):
    """k >= 2 code lengths of a complete code by random Kraft splitting: a leaf becomes two leaves one level down."""
    assert 2 <= k <= (1 << maxbits)
    leaves, p_deep = [1, 1], rng.choice((0.1, 0.5, 0.9))   # p_deep: how often the newest (a deepest) leaf is the one split
    while len(leaves) < k:
        i = len(leaves) - 1 if rng.random() < p_deep else rng.randrange(len(leaves))
        if leaves[i] >= maxbits:
            i = min(range(len(leaves)), key=leaves.__getitem__)
        d = leaves[i]
        leaves[i] = d + 1
        leaves.append(d + 1)
    rng.shuffle(leaves)
    return leaves


def _random_code(rng, used, n_symbols, lo, maxbits=15):
    """a complete code over `used` (>= 1 symbol) and, if it has one symbol only or by chance, a few unused symbols"""
    syms = set(used)
    spare = [s for s in range(n_symbols) if s not in syms]
    for _ in range((2 - len(syms)) if len(syms) < 2 else rng.choice((0, 0, 1, 3, len(spare) // 2))):
        syms.add(spare.pop(rng.randrange(len(spare))))
    n = rng.randint(max(max(syms) + 1, lo), n_symbols)
    out = [0] * n
    for s, l in zip(sorted(syms), random_complete_lengths(rng, len(syms), maxbits)):
        out[s] = l
    return out


def _apply(out, tokens):
    for t in tokens:
        if type(t) is Lit:
            out.append(t.byte)
        else:
            for _ in range(t.length):
                out.append(out[-t.distance])


F_MEMBERS = 1500


@functools.lru_cache(None)
def family_f(n_members=F_MEMBERS, seed=77):
    rng = random.Random(seed)
    members = []
    for i in range(n_members):
        size = rng.choice((0, 1, 2, 3, 64, 257, 2048)) if rng.random() < 0.1 else rng.randrange(0, 2049)
        alphabet, p_match = rng.choice((1, 2, 4, 16, 64, 256)), rng.choice((0.0, 0.1, 0.3, 0.6, 0.9))
        toks, pos = [], 0
        while pos < size:
            if pos and size - pos >= 3 and rng.random() < p_match:
                r = rng.random()
                length = rng.randint(3, 10) if r < 0.5 else rng.randint(3, 258) if r < 0.8 else 258 if r < 0.9 else \
                    (lambda k: LEN_BASE[k] + rng.randrange(1 << LEN_EXTRA[k]))(rng.randrange(29))
                length = min(length, size - pos)
                r = rng.random()   # any distance up to the bytes so far is legal, the shorter-than-length (self-overlapping) ones too
                dist = rng.randint(1, min(pos, 8)) if r < 0.4 else rng.randint(1, pos) if r < 0.8 else max(1, pos - rng.randrange(2))
                toks.append(Match(length, dist, length == 258 and rng.random() < 0.5))
                pos += length
            else:
                toks.append(Lit(rng.randrange(alphabet) * (256 // alphabet)))
                pos += 1
        cuts = sorted(rng.randrange(len(toks) + 1) for _ in range(rng.choice((0, 0, 1, 2, 5))))
        w, regimes = DeflateWriter(), set()
        chunks = [toks[a:b] for a, b in zip([0] + cuts, cuts + [len(toks)])]
        for bi, chunk in enumerate(chunks):
            final = bi == len(chunks) - 1
            kind = rng.choice(("stored", "fixed", "dynamic", "dynamic"))
            if kind == "stored":
                tmp = bytearray(w.out)
                _apply(tmp, chunk)
                w.stored(bytes(tmp[len(w.out):]), final)
                continue
            if kind == "fixed":
                w.begin_fixed(final)
            else:
                lsyms = {256} | {t.byte if type(t) is Lit else length_symbol(t.length, t.alt258)[0] for t in chunk}
                dsyms = {distance_symbol(t.distance)[0] for t in chunk if type(t) is Match}
                if lsyms == {256} and rng.random() < 0.5:
                    ll = list(EOB_ONLY_LL)
                    regimes.add("single litlen code")
                else:
                    ll = _random_code(rng, lsyms, 286, 257)
                if not dsyms and rng.random() < 0.6:
                    dl = [0] * rng.randint(1, 30)
                    regimes.add("no distance code")
                elif len(dsyms) <= 1 and rng.random() < 0.6:
                    s = min(dsyms) if dsyms else rng.randrange(30)
                    dl = [0] * s + [1] + [0] * rng.randrange(30 - s)
                    regimes.add("single distance code")
                else:
                    dl = _random_code(rng, dsyms or {rng.randrange(30)}, 30, 1)
                rle = rng.choice(("none", "greedy"))
                seq = ll + dl
                used = {s for s, _ in ([(l, 0) for l in seq] if rle == "none" else rle_greedy(seq))}
                cl = [0] * 19
                if rng.random() < 0.5:
                    cl_syms = sorted(used) if len(used) > 1 else sorted(used | {0 if 0 not in used else 1})
                    for s, l in zip(cl_syms, random_complete_lengths(rng, len(cl_syms), 7)):
                        cl[s] = l
                else:
                    cl = balanced_lengths(used)
                need = max([k + 1 for k in range(19) if cl[CL_ORDER[k]]] + [4])
                w.begin_dynamic(ll, dl, Header(cl, rng.choice((need, 19, rng.randint(need, 19))), rle), final)
            w.put(chunk)
            w.end_block()
        members.append(Member(f"F/{i}", w.payload(), bytes(w.out), None, blocks=w.blocks, regimes=regimes))
    # two or three launches on the device: files of 600 members
    return [build_file(members[a:a + 600]) for a in range(0, n_members, 600)]
