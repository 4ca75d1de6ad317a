"""bgzf_inflate_kernel on DEFLATE streams zlib's compressor never writes: the families of tests/deflate_synth.py, whose
reach tests/test_deflate_cpu.py proves from the reference alone.  Expected bytes are zlib's (`zlib.decompressobj(-15)`), the CRC check
of pisces_hip_bgzf_inflate stays on.

  positive   each family is one file and one launch (F: three); a failure names the member and its first differing byte.
  negative   every row of family E between two valid members: the error names block 1 and the status bgzf_kernels.hip.h documents
             for it; the handle then inflates family A again.
  agreement  200 seeded single-field mutations of the headers of family B's dynamic blocks: the device accepts exactly those zlib
             accepts with the CRC still matching, and gives zlib's bytes for them.

Seen to fail against a library with one line of bgzf_kernels.hip.h changed (on an MI355X, the repository untouched; an inflate error
names the first bad block of a launch only):
  `t < 64u ? from_x : from_y` as `t <= 64u`            A/eob4/blocks0-31, B/all_symbols_fixed, C/pair/dynamic-dynamic/0, F/4
  `pair_bytes <= 64` as `<= 65`                         D/pair_bytes65, F/113
  the 0x1FF length mask of prepare() as 0xFF            B/maximal_header, D/overlap258_distance1, F/2
  the distance code's single-code exemption removed     B/single_distance_code, F/1
  long distance code's extra bits read one bit early    A/eob12/blocks0-31, F/166
`pair_bytes <= 64` as `< 64` changes no byte (the pair-by-pair loop takes over), so no member can see it.
Measured there: family F 1.2 s, family A 0.3 s, every other test 0.1 s or less."""
import re
import zlib

import numpy as np
import pytest

from pisces_amd import _abi, engine
from tests import deflate_synth as ds
from tests.test_deflate_cpu import files_of
from tests.test_read_store import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def _check_file(c, f):
    """failures of one file as strings: member and first differing byte"""
    got, blocks, _ = c.bgzf_inflate(f.data)
    assert len(blocks) == len(f.members) + 1 and len(got) == f.table[-1][2]
    bad = []
    for m, (_, _, at, isize, _) in zip(f.members, f.table):
        want, have = zlib.decompressobj(-15).decompress(m.payload), got[at:at + isize]
        if have != want:
            first = next((i for i, (a, b) in enumerate(zip(have, want)) if a != b), min(len(have), len(want)))
            bad.append(f"{m.name}: first differing byte {first} of {len(want)} (got {have[first:first + 1].hex()}, zlib {want[first:first + 1].hex()})")
    return bad


def _inflate_family(c, name):
    bad = []
    for f in files_of(name):
        try:
            bad += _check_file(c, f)
        except engine.PiscesHipError as e:   # the error names a block of the file: say which member that is
            k = re.search(r"block (\d+)", str(e))
            who = f.members[int(k.group(1))].name if k and int(k.group(1)) < len(f.members) else "?"
            bad.append(f"{who}: {e}")
    return bad


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F"])
def test_device_inflate_of_a_family_equals_zlib(torch_cuda, name):
    with engine.HipVariantCaller(_abi.default_config()) as c:
        bad = _inflate_family(c, name)
    assert not bad, "%d members differ:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_negative_table_is_refused_with_the_documented_status(torch_cuda):
    rows, bad = ds.family_e(), []
    with engine.HipVariantCaller(_abi.default_config()) as c:
        for r in rows:
            f = ds.negative_file(r)
            try:
                c.bgzf_inflate(f.data)
                bad.append(f"{r.name}: accepted")
                continue
            except engine.PiscesHipError as e:
                msg = str(e)
            print(r.name, "->", msg)
            k = re.search(r"block (\d+) is not a valid DEFLATE stream of its ISIZE \(code (\d+)\)", msg)
            if not k or int(k.group(1)) != 1 or int(k.group(2)) == 0 or (r.status is not None and int(k.group(2)) != r.status):
                bad.append(f"{r.name}: expected block 1, code {r.status}: {msg}")
        assert not bad, "\n".join(bad)
        assert not _inflate_family(c, "A")   # the handle has survived the whole table


def _set_bits(payload, bit, width, value):
    v = int.from_bytes(payload, "little")
    v = (v & ~(((1 << width) - 1) << bit)) | (value << bit)
    return v.to_bytes(len(payload), "little")


def header_mutations(n=200, seed=5):
    """(member, mutated payload, what): one of HLIT / HDIST / HCLEN / one code-length-code length of a dynamic block of family B set to
    another value"""
    rng = np.random.default_rng(seed)
    sites = [(m, i, b["fields"]) for m in ds.family_b().members for i, b in enumerate(m.blocks) if b["kind"] == "dynamic"]
    out = []
    for _ in range(n):
        m, i, fields = sites[int(rng.integers(len(sites)))]
        which = ("hlit", "hdist", "hclen", "cl")[int(rng.integers(4))]
        bit, width = (fields[which], {"hlit": 5, "hdist": 5, "hclen": 4}[which]) if which != "cl" else (fields["cl"][int(rng.integers(len(fields["cl"])))], 3)
        old = (int.from_bytes(m.payload, "little") >> bit) & ((1 << width) - 1)
        new = (old + 1 + int(rng.integers((1 << width) - 1))) % (1 << width)
        out.append((m, _set_bits(m.payload, bit, width, new), f"{m.name} block {i} {which} at bit {bit}: {old} -> {new}"))
    return out


def test_device_and_zlib_agree_on_mutated_dynamic_headers(torch_cuda):
    bad, accepted = [], 0
    with engine.HipVariantCaller(_abi.default_config()) as c:
        for m, payload, what in header_mutations():
            assert payload != m.payload and len(payload) == len(m.payload)
            data = m.data
            try:
                out, eof = ds.zlib_inflate(payload)
                ref = out if eof and len(out) == len(data) and zlib.crc32(out) == zlib.crc32(data) else None
            except zlib.error:
                ref = None
            f = ds.build_file([ds.Member(m.name, payload, None, m.in_offset % 16, len(data), zlib.crc32(data))])
            try:
                got, _, _ = c.bgzf_inflate(f.data)
            except engine.PiscesHipError as e:
                got = None
                assert "block 0" in str(e), str(e)
            accepted += ref is not None
            if (got is None) != (ref is None) or (ref is not None and got != ref):
                bad.append(f"{what}: zlib {'accepts' if ref is not None else 'refuses'}, the device {'accepts' if got is not None else 'refuses'}"
                           + (" other bytes" if got is not None and ref is not None else ""))
    print(f"{accepted} of 200 mutated headers are still accepted by zlib")
    assert not bad, "\n".join(bad)
