"""pisces_hip_format_vcf_device on the GPU: every comparison is device bytes == host bytes, the host formatter (engine.format_vcf,
pinned to the lines Pisces wrote by tests/test_vcf_format.py) being the yardstick.  DESIGN.md 3.12 says which one-line changes of the
kernels each test catches."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pisces_amd import _abi
from tests import vcf_device_cases as cases
from tests import test_vcf_format as host_tests

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def caller(torch_cuda):
    from pisces_amd import engine
    with engine.HipVariantCaller(_abi.default_config()) as c:
        yield c


def vcf_config(**kw):
    from pisces_amd import engine
    cfg = _abi.PiscesVcfConfig()
    assert engine.lib.pisces_hip_vcf_default_config(C.byref(cfg)) == 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def host_text(chrom, rows, alleles=None, gp=None, **kw):
    from pisces_amd import engine
    return engine.format_vcf(chrom, rows, alleles=alleles, posteriors=gp, **kw).encode()


def candidates_of(alleles):
    """cand_index / cands / pool as engine.format_vcf builds them from (ref, alt) pairs: numpy byte arrays"""
    idx, cands, pool = [], [], bytearray()
    for (r, a) in alleles:
        if len(r) == 1 and len(a) == 1:
            idx.append(-1)
            continue
        c = _abi.PiscesCandidate()
        c.ref_len, c.alt_len, c.allele_offset = len(r), len(a), len(pool)
        pool += r.encode() + a.encode()
        idx.append(len(cands))
        cands.append(bytes(c))
    return (np.array(idx, dtype=np.int32), np.frombuffer(b"".join(cands) or b"\0", dtype=np.uint8).copy(), np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy())


def upload(torch, c, arr):
    """a numpy array as device bytes, made on the handle's stream"""
    with torch.cuda.stream(c.torch_stream()):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", c.device))


def raw_format(torch, c, chrom, rows, cfg, n=None, count=None, alleles=None, gp=None, capacity=None, offsets=False, cands_null=False):
    """One pisces_hip_format_vcf_device call with a sentinel-filled text buffer: (rc, size word, whole text buffer, offsets or None)"""
    from pisces_amd import engine
    ts = c.torch_stream()
    dev = torch.device("cuda", c.device)
    n = len(rows) if n is None else n
    d_rows = upload(torch, c, rows) if len(rows) else None
    d_idx = d_cands = d_pool = d_gp = d_count = d_offs = None
    if alleles is not None:
        idx, cands, pool = candidates_of(alleles)
        d_idx = upload(torch, c, idx)
        if not cands_null:
            d_cands, d_pool = upload(torch, c, cands), upload(torch, c, pool)
    if gp is not None:
        d_gp = upload(torch, c, gp)
    with torch.cuda.stream(ts):
        if count is not None:
            d_count = torch.tensor([count], dtype=torch.int32, device=dev)
        if offsets:
            d_offs = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        text = torch.full((max(capacity, 0) + 64,), SENTINEL, dtype=torch.uint8, device=dev)
        word = torch.full((1,), -99, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    rc = engine.lib.pisces_hip_format_vcf_device(c._h, C.byref(cfg), chrom.encode(), p(d_rows), n, p(d_count), p(d_idx), p(d_cands), p(d_pool), p(d_gp),
                                                 text.data_ptr(), capacity, p(d_offs), word.data_ptr(), None)
    c.synchronize()
    return rc, int(word.cpu()[0]), text.cpu().numpy(), (d_offs.cpu().numpy() if offsets else None)


def device_text(torch, c, chrom, rows, alleles=None, gp=None, **kw):
    """engine.format_vcf_device on uploaded rows"""
    d_rows = upload(torch, c, rows) if len(rows) else None
    extra = {}
    if alleles is not None:
        idx, cands, pool = candidates_of(alleles)
        extra = dict(d_cand_index=upload(torch, c, idx), d_cands=upload(torch, c, cands), d_alleles=upload(torch, c, pool))
    if gp is not None:
        extra["d_gp"] = upload(torch, c, gp)
    return c.format_vcf_device(chrom, d_rows, len(rows), **extra, **kw)


@pytest.mark.parametrize("spec", json.load(open(os.path.join(GOLDEN, "vcf_lines.json"))), ids=lambda s: os.path.basename(s["file"]))
def test_lines_pisces_wrote_come_out_of_the_device(torch_cuda, caller, spec):
    """Every parsable line of a reference test-data VCF (what test_lines_pisces_wrote_are_reproduced parses), with the file's filter
    configuration and the line's own columns and decimals, as one batch per configuration of the file."""
    batches = {}
    for line in spec["lines"]:
        parsed = host_tests._parse(line, spec)
        if parsed is None:
            continue
        r, alleles, f, decimals = parsed
        kw = dict(variant_quality_filter=spec["q"] if spec["q"] is not None else -1,
                  rmxn_max_repeat_length=spec["rmxn"][0] if spec["rmxn"] else -1, rmxn_min_repetitions=spec["rmxn"][1] if spec["rmxn"] else -1,
                  noise_level=int(f["NL"]) if "NL" in f else 20, output_strand_bias_and_noise_level=int("NL" in f),
                  output_no_call_fraction=int("NC" in f), min_frequency_threshold=10.0 ** -(decimals - 1), frequency_filter_threshold=-1.0)
        b = batches.setdefault((line.split("\t")[0],) + tuple(sorted(kw.items())), ([], [], kw))
        b[0].append(r)
        b[1].append(alleles)
    checked = 0
    for key, (rows, alleles, kw) in batches.items():
        rows = np.concatenate(rows)
        want = host_text(key[0], rows, alleles=alleles, **kw)
        got = device_text(torch_cuda, caller, key[0], rows, alleles=alleles, **kw)
        assert got == want, (key[0], kw)
        checked += len(rows)
    assert checked >= (7 * len(spec["lines"])) // 10


CONFIGS = {
    "default": {},
    "five_decimals": dict(frequency_filter_threshold=1e-5),
    "no_nl_sb": dict(output_strand_bias_and_noise_level=0),
    "nc": dict(output_no_call_fraction=1),
    "nl_from_records": dict(noise_level_from_records=1),
}


def first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for k, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return k, a, b
    return min(len(g), len(w)), None, None


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seeded_rows_under_five_configurations(torch_cuda, caller, name):
    rows, gps, stats = cases.cases()
    want = host_text("chr7", rows, gp=gps, **CONFIGS[name])
    got = device_text(torch_cuda, caller, "chr7", rows, gp=gps, **CONFIGS[name])
    assert got == want, first_difference(got, want)
    if name == "default":   # and without the GP column
        assert device_text(torch_cuda, caller, "chr7", rows) == host_text("chr7", rows)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_row_counts_across_waves_and_workgroups(torch_cuda, caller, n):
    rows, gps, stats = cases.cases()
    rows, gps = rows[:n], gps[:n]
    want = host_text("chr1", rows, gp=gps)
    rc, word, text, offs = raw_format(torch_cuda, caller, "chr1", rows, vcf_config(), gp=gps if n else None, capacity=len(want), offsets=True)
    assert rc == 0 and word == len(want)
    assert text[:len(want)].tobytes() == want and (text[len(want):] == SENTINEL).all()
    starts = np.cumsum([0] + [len(l) + 1 for l in want.split(b"\n")[:-1]])
    assert offs.tolist() == starts.tolist()   # rows + 1 entries: every line's offset, then the total


@pytest.mark.parametrize("count", [0, 100, 4097, 9999])
def test_the_count_word_bounds_the_rows(torch_cuda, caller, count):
    rows, gps, stats = cases.cases()
    rows = rows[:4097]
    want = host_text("chr1", rows[:min(count, len(rows))])
    rc, word, text, offs = raw_format(torch_cuda, caller, "chr1", rows, vcf_config(), count=count, capacity=len(want) + 7, offsets=True)
    assert rc == 0 and word == len(want)
    assert text[:len(want)].tobytes() == want and (text[len(want):] == SENTINEL).all()
    k = min(count, len(rows))
    assert offs[k] == len(want) and (offs[k + 1:] == -1).all()


def test_allele_strings_through_the_lds_chunk_and_the_long_path(torch_cuda, caller):
    """Candidate rows of 1 / 63 / 64 / 300-byte alleles among point rows (their waves still fit the LDS chunk), then the same candidate
    rows alone (64 lines of several hundred bytes: the byte path), then a 336-byte chrom (every wave on the byte path)."""
    rows, alleles = cases.allele_cases()
    assert device_text(torch_cuda, caller, "chr2", rows, alleles=alleles) == host_text("chr2", rows, alleles=alleles)
    long_ones = [k for k, (r, a) in enumerate(alleles) if len(r) + len(a) > 100]
    dense_rows = np.concatenate([rows[long_ones]] * 12)
    dense_alleles = [alleles[k] for k in long_ones] * 12
    assert len(dense_rows) > 128
    want = host_text("chr2", dense_rows, alleles=dense_alleles)
    assert len(want) > 200 * len(dense_rows)
    assert device_text(torch_cuda, caller, "chr2", dense_rows, alleles=dense_alleles) == want
    chrom = "chrUn_" + "scaffold_with_a_long_name_" * 12 + "end_of_name_xyz123"
    assert len(chrom) == 336
    plain, gps, stats = cases.cases()
    assert device_text(torch_cuda, caller, chrom, plain[:300], gp=gps[:300]) == host_text(chrom, plain[:300], gp=gps[:300])


def test_capacity_protocol(torch_cuda, caller):
    rows, gps, stats = cases.cases()
    rows = rows[:1000]
    want = host_text("chr1", rows)
    need = len(want)
    rc, word, text, _ = raw_format(torch_cuda, caller, "chr1", rows, vcf_config(), capacity=need - 1)
    assert rc == 0 and word == need and (text == SENTINEL).all()          # one byte short: the size, and not a byte written
    rc, word, text, _ = raw_format(torch_cuda, caller, "chr1", rows, vcf_config(), capacity=0)
    assert rc == 0 and word == need and (text == SENTINEL).all()
    rc, word, text, _ = raw_format(torch_cuda, caller, "chr1", rows, vcf_config(), capacity=need)
    assert rc == 0 and word == need and text[:need].tobytes() == want      # exactly fitting
    assert (text[need:] == SENTINEL).all()                                 # and the byte behind the text is untouched
    # the engine entry grows its buffer once
    d_rows = upload(torch_cuda, caller, rows)
    assert caller.format_vcf_device("chr1", d_rows, len(rows), capacity=100) == want


def test_text_into_pinned_host_memory_and_offsets_through_the_engine(torch_cuda, caller):
    """d_text and the size word in pinned host memory (the kernels' own stores cross the bus, as the flush's rows do), an odd start
    address so that the chunks' head and tail bytes differ from the aligned case; and engine.format_vcf_device's line_offsets."""
    from pisces_amd import engine
    torch = torch_cuda
    rows, gps, stats = cases.cases()
    rows = rows[:777]
    want = host_text("chr1", rows)
    pinned = torch.full((len(want) + 64,), SENTINEL, dtype=torch.uint8).pin_memory()
    word = torch.full((1,), -99, dtype=torch.int64).pin_memory()
    d_rows = upload(torch, caller, rows)
    cfg = vcf_config()
    for skew in (0, 5):
        pinned.fill_(SENTINEL)
        rc = engine.lib.pisces_hip_format_vcf_device(caller._h, C.byref(cfg), b"chr1", d_rows.data_ptr(), len(rows), None, None, None, None, None,
                                                     pinned.data_ptr() + skew, len(want), None, word.data_ptr(), None)
        caller.synchronize()
        got = pinned.numpy()
        assert rc == 0 and int(word[0]) == len(want)
        assert got[skew:skew + len(want)].tobytes() == want and (got[:skew] == SENTINEL).all() and (got[skew + len(want):] == SENTINEL).all()
    text, offs = caller.format_vcf_device("chr1", d_rows, len(rows), line_offsets=True)
    assert text == want and len(offs) == len(rows) + 1 and offs[-1] == len(want)
    assert all(text[int(o) - 1:int(o)] == b"\n" for o in offs[1:])
    # with a count word below n the entry hands back the rows + 1 entries the kernels wrote, whatever bytes the text holds
    with torch.cuda.stream(caller.torch_stream()):
        d_count = torch.tensor([100], dtype=torch.int32, device="cuda")
    text, offs = caller.format_vcf_device("chr1", d_rows, len(rows), d_count=d_count, line_offsets=True)
    short = host_text("chr1", rows[:100])
    assert text == short and len(offs) == 101 and offs[0] == 0 and offs[-1] == len(short)


def _plain(n=200):
    rows, gps, stats = cases.cases()
    ok = rows[(rows["filter_bits"] & cases.ALL_FILTERS) == 0][:n].copy()
    assert len(ok) == n
    return ok


def _host_rc(chrom, rows, cfg, alleles=None, cands_null=False):
    from pisces_amd import engine
    idx = cands = pool = None
    if alleles is not None:
        idx, cands, pool = candidates_of(alleles)
    buf = C.create_string_buffer(1 << 20)
    return int(engine.lib.pisces_hip_format_vcf_ex(C.byref(cfg), chrom.encode(), rows.ctypes.data, len(rows), idx.ctypes.data if idx is not None else None,
                                                   None if (cands is None or cands_null) else cands.ctypes.data,
                                                   None if (pool is None or cands_null) else pool.ctypes.data, buf, 1 << 20, None))


@pytest.mark.parametrize("kind", ["qscore", "rmxn", "candidates", "two_kinds"])
def test_rows_the_host_formatter_refuses(torch_cuda, caller, kind):
    """The host entry's code and no text.  Every refusal the host formatter can reach is PISCES_E_INVALID_ARG (its PISCES_E_INTERNAL branch
    is behind a loop over the named bits only), so WHICH of two offending rows decided cannot be seen in the size word: two_kinds checks
    that two rows of different kinds still give the host's code and not a byte of text, not which of them the device took."""
    rows = _plain()
    cfg = vcf_config()
    alleles = None
    cands_null = False
    if kind == "qscore":
        cfg.variant_quality_filter = -1
        rows["filter_bits"][[150, 70]] |= 1 << 3
    elif kind == "rmxn":
        cfg.rmxn_min_repetitions = -1
        rows["filter_bits"][[199, 3]] |= 1 << 9
    elif kind == "candidates":
        alleles = [("A", "T")] * len(rows)
        alleles[120] = ("A", "ATT")
        alleles[64] = ("ACG", "A")
        cands_null = True
    else:   # an RMxN row in front of a q-score row, both unnamed: row 10 decides
        cfg.variant_quality_filter = -1
        cfg.rmxn_max_repeat_length = -1
        rows["filter_bits"][10] |= 1 << 9
        rows["filter_bits"][11] |= 1 << 3
    want = _host_rc("chr1", rows, cfg, alleles, cands_null)
    assert want == _abi.E_INVALID_ARG
    rc, word, text, offs = raw_format(torch_cuda, caller, "chr1", rows, cfg, alleles=alleles, capacity=1 << 16, offsets=True, cands_null=cands_null)
    assert rc == 0 and word == want and (text == SENTINEL).all() and (offs == -1).all()
    from pisces_amd import engine
    with pytest.raises(engine.PiscesHipError) as e:
        caller.format_vcf_device("chr1", upload(torch_cuda, caller, rows), len(rows), vcf_config=cfg,
                                 **({} if alleles is None else dict(d_cand_index=upload(torch_cuda, caller, candidates_of(alleles)[0]))))
    assert e.value.code == want


def test_a_filter_bit_without_a_name_is_what_the_host_makes_of_it(torch_cuda, caller):
    """Bits 1, 7, 11 and 13 have no VCF name.  The host formatter's loop runs over the named bits only, so its PISCES_E_INTERNAL branch
    is never reached and such a bit prints nothing; the device does the same: the same code (none) and the same bytes."""
    rows = _plain()
    for k, b in enumerate((1, 7, 11, 13)):
        rows["filter_bits"][10 + k] |= 1 << b
    rows["filter_bits"][20] |= (1 << 1) | (1 << 4)
    assert _host_rc("chr1", rows, vcf_config()) > 0
    want = host_text("chr1", rows)
    assert device_text(torch_cuda, caller, "chr1", rows) == want
    assert want.split(b"\n")[20].split(b"\t")[6] == b"LowDP"


def test_refusals_at_the_call(torch_cuda, caller):
    from pisces_amd import engine
    rows = _plain(10)
    d_rows = upload(torch_cuda, caller, rows)
    with pytest.raises(engine.PiscesHipError) as e:
        caller.format_vcf_device("chr1", d_rows, len(rows), crush=1)
    assert e.value.code == _abi.E_UNSUPPORTED and "crush" in str(e.value)
    with pytest.raises(engine.PiscesHipError) as e:
        caller.format_vcf_device("c" * 1025, d_rows, len(rows))
    assert e.value.code == _abi.E_UNSUPPORTED
    with pytest.raises(engine.PiscesHipError) as e:
        caller.format_vcf_device("chr1", d_rows, len(rows), min_frequency_threshold=1e-8)
    assert e.value.code == _abi.E_UNSUPPORTED
    cfg = vcf_config()
    word = torch_cuda.zeros(1, dtype=torch_cuda.int64, device="cuda")
    lib = engine.lib
    assert lib.pisces_hip_format_vcf_device(caller._h, C.byref(cfg), b"chr1", d_rows.data_ptr(), -1, None, None, None, None, None, None, 0, None, word.data_ptr(), None) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_format_vcf_device(caller._h, C.byref(cfg), b"chr1", d_rows.data_ptr(), 1, None, None, None, None, None, None, 0, None, None, None) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_format_vcf_device(caller._h, C.byref(cfg), None, d_rows.data_ptr(), 1, None, None, None, None, None, None, 0, None, word.data_ptr(), None) == _abi.E_INVALID_ARG
    assert lib.pisces_hip_format_vcf_device(caller._h, None, b"chr1", d_rows.data_ptr(), 1, None, None, None, None, None, None, 0, None, word.data_ptr(), None) == _abi.E_INVALID_ARG
    with pytest.raises(ValueError):   # the null stream, as everywhere on this surface
        caller.format_vcf_device("chr1", d_rows, len(rows), stream=0)
    # the most decimals the device takes
    seven = dict(min_frequency_threshold=1e-7)
    plain, gps, stats = cases.cases()
    assert device_text(torch_cuda, caller, "chr1", plain[:2000], **seven) == host_text("chr1", plain[:2000], **seven)


def _tiles_of_the_small_golden(torch, c):
    z = np.load(os.path.join(GOLDEN, "synthetic_small.npz"))
    order = np.argsort(z["positions"], kind="stable")
    pos, tup = z["positions"][order], z["tuples"][order]
    start, n_loci = int(z["region_start"]), int(z["n_loci"])
    n_tiles = (n_loci + 63) // 64
    tiles = np.zeros(n_tiles, dtype=_abi.TILE_DTYPE)
    for t in range(n_tiles):
        a = start + 64 * t
        b = min(a + 64, start + n_loci)
        tiles[t] = (a, b - a, np.searchsorted(pos, a), np.searchsorted(pos, b))
    return z, upload(torch, c, tup), upload(torch, c, tiles), n_tiles, upload(torch, c, z["ref"])


def _call_compact_format(torch, c, adaptive):
    """call_tiles -> compact_records (-> compact_posteriors) -> format_vcf_device on one stream, no host wait in between"""
    from pisces_amd import engine
    z, d_tup, d_tiles, n_tiles, d_ref = _tiles_of_the_small_golden(torch, c)
    ts = c.torch_stream()
    dev = torch.device("cuda", c.device)
    cap = n_tiles * _abi.SLOTS_PER_TILE
    with torch.cuda.stream(ts):
        recs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
        tres = torch.zeros(n_tiles * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        out_d = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
        offs = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        post = torch.zeros(cap * 32, dtype=torch.uint8, device=dev) if adaptive else None
        post_d = torch.zeros(cap * 32, dtype=torch.uint8, device=dev) if adaptive else None
        text = torch.full((cap * 160,), SENTINEL, dtype=torch.uint8, device=dev)
        word = torch.full((1,), -99, dtype=torch.int64, device=dev)
    cfg = vcf_config()
    c.synchronize()
    c.call_tiles(d_tup.data_ptr(), d_tiles.data_ptr(), n_tiles, d_ref.data_ptr(), 1, len(z["ref"]), recs.data_ptr(), cap, tres.data_ptr(), ts, posteriors=post)
    c.compact_records(recs.data_ptr(), tres.data_ptr(), n_tiles, offs.data_ptr(), out_d.data_ptr(), cap, count.data_ptr(), ts)
    if adaptive:
        c.compact_posteriors(post.data_ptr(), tres.data_ptr(), n_tiles, offs.data_ptr(), post_d.data_ptr(), cap, ts)
    rc = engine.lib.pisces_hip_format_vcf_device(c._h, C.byref(cfg), b"chr19", out_d.data_ptr(), cap, count.data_ptr(), None, None, None,
                                                 post_d.data_ptr() if adaptive else None, text.data_ptr(), text.numel(), None, word.data_ptr(), ts.cuda_stream)
    assert rc == 0
    c.synchronize()
    n = int(count.cpu()[0])
    rows = out_d.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy()
    gp = post_d.cpu().numpy().view(_abi.POSTERIORS_DTYPE)[:n].copy() if adaptive else None
    need = int(word.cpu()[0])
    return rows, gp, text.cpu().numpy()[:max(need, 0)].tobytes(), need


def test_end_to_end_from_tuples_to_text(torch_cuda, caller):
    rows, _, text, need = _call_compact_format(torch_cuda, caller, adaptive=False)
    assert len(rows) > 900
    want = host_text("chr19", rows)
    assert need == len(want) and text == want
    again = _call_compact_format(torch_cuda, caller, adaptive=False)
    assert again[2] == text   # two runs, the same bytes


def test_end_to_end_with_an_adaptive_handle_and_gp(torch_cuda):
    from pisces_amd import engine
    cfg = _abi.default_config(ploidy=_abi.PLOIDY_DIPLOID_ADAPTIVE, min_frequency=0.0, low_gq_filter=30)
    with engine.HipVariantCaller(cfg) as c:
        rows, gp, text, need = _call_compact_format(torch_cuda, c, adaptive=True)
    assert len(rows) > 900 and (gp["n"] > 0).any()
    want = host_text("chr19", rows, gp=gp)
    assert b":GP\t" in want
    assert need == len(want) and text == want
