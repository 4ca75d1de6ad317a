"""What lives for one flush stays in that flush (FlushScope, surface_flush.inc.h): the dirty-locus window, refs_only, the folded-count window,
variants_only / totals of the off-interval counting launch.  The handle's parameters are what pisces_hip_create made of them, so a direct
tile call gives the same rows whatever was flushed before it, a flush that is refused half way leaves nothing behind, and a flush does not
see the windows of the one before it.  The direct calls use the nine-tile grids of tests/test_tile_launch_args_gpu.py, the streaming side
1000-locus blocks of a few hundred reads.
"""
import numpy as np
import pytest

from pisces_amd import _abi
from tests import orc
from tests.test_read_store import env, torch_cuda  # noqa: F401
from tests.test_tile_launch_args_gpu import CELLS, check, grid_of, view_of
from tests.test_tuple_geometry_gpu import FORMS, NO_SWITCH

pytestmark = pytest.mark.gpu
BLOCK_FORM = FORMS[0]             # call_tiles_kernel: DeviceParams by value
KERNEL_FORMS = ["wave", "wave2", BLOCK_FORM]
READ_PATHS = {"store": None, "log": "log"}
INTERVALS = [(200, 420), (1100, 1180), (2050, 2300)]
_CACHE = {}


def _eqx(reads, ref):
    """Every third read of one M operation with that operation written as runs of = and X."""
    out = []
    for i, r in enumerate(reads):
        if i % 3 or len(r["cigar"]) != 1:
            out.append(r)
            continue
        ops = []
        for k, b in enumerate(r["seq"].encode()):
            t = "=" if b == ref[r["pos"] - 1 + k] else "X"
            if ops and ops[-1][0] == t:
                ops[-1] = (t, ops[-1][1] + 1)
            else:
                ops.append((t, 1))
        out.append(dict(r, cigar=ops) if len(ops) > 1 else r)   # (a read that equals the reference stays as it is)
    return out


def streaming_input(blocks, eqx=False):
    """One 1000-locus block per letter: 'm' ~300 reads of tests.test_gpu_parity._mnv_reads (MNVs, SNVs, a few indels), 'p' 100 reads that
    equal the reference.  Reads stay inside their block."""
    key = (blocks, eqx)
    if key not in _CACHE:
        from tests.test_gpu_parity import _mnv_reads
        rng = np.random.default_rng(4711)
        ref = bytes(rng.choice(list(b"ACGT"), 1000 * len(blocks)).astype(np.uint8))
        reads = []
        for k, kind in enumerate(blocks):
            lo = 1000 * k + 1
            if kind == "m":
                reads += _mnv_reads(rng, ref, 300, read_len=90, region=(lo + 6, lo + 993))
            else:
                for i, start in enumerate(rng.integers(lo + 6, lo + 900, 100).tolist()):
                    reads.append({"pos": start, "cigar": [("M", 90)], "seq": ref[start - 1: start + 89].decode(), "quals": [37] * 90, "reverse": bool(i % 2)})
        reads.sort(key=lambda r: r["pos"])
        if eqx:
            reads = _eqx(reads, ref)
            assert sum(op == "X" for r in reads for op, _ in r["cigar"]) >= 20
        _CACHE[key] = (np.frombuffer(ref, dtype=np.uint8), reads)
    return _CACHE[key]


def flush_in_every_form(c, refa, reads):
    """Call(upTo) over the first block, CallBegin / CallEnd over the second (no candidate in it: the device alone), Call() over the third."""
    c.SetReference(refa)
    c.AddAlleleCounts(_abi.ReadBatch(reads))
    rows = [c.Call(upToPosition=1000)]
    c.CallBegin(upToPosition=2000)
    rows.append(c.CallEnd())
    rows.append(c.Call())
    assert all(len(r) for r in rows) and rows[0]["position"].max() <= 1000 < rows[1]["position"].min() <= rows[1]["position"].max() <= 2000 < rows[2]["position"].min()


# name: configuration, reads with X / = operations, interval set + exact TotalNumCalled, the direct calls against the oracle
CASES = {
    "default": (dict(), True, False, True),
    "mnv": (dict(call_mnvs=1), False, False, False),
    "exact total": (dict(), True, True, True),
    "snv walk": (dict(collapse_freq_ratio_threshold=1.0), False, False, True),
}
RUNS = ([("default", f, p) for f in KERNEL_FORMS for p in READ_PATHS] + [("mnv", f, p) for f in KERNEL_FORMS for p in READ_PATHS] +
        [("exact total", f, "store") for f in ("wave", "wave2")] +      # (the counting launch is the read store's fused kernel's)
        [("snv walk", f, "store") for f in KERNEL_FORMS])


@pytest.mark.parametrize("case,form,path", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_direct_tile_calls_are_blind_to_flushes(torch_cuda, case, form, path):
    """pisces_hip_call_tiles on one handle before and after a streaming run that goes through every form of the flush.
    default: reads with X / = operations, so the flushes of MNV calling off have dirty loci; both direct calls give the oracle's rows.
    mnv: the split form (dirty loci, a folded window, refs_only 0 inside the flushes, 1 outside); the second call's bytes are the first's.
    exact total: an interval set and pisces_hip_set_exact_total_called, so a variants_only launch without totals runs in between.
    snv walk: MNV calling off with collapser thresholds that take the SNV candidates from the read walk — a flush runs with refs_only 1
    (0 in the split form) and the handle was created with 0.  That the direct call keeps the create-time value after a flush is what this
    change pins: before it the second call of this case gave Reference rows only."""
    from pisces_amd import engine
    from tests.test_gpu_parity import run_fused
    kw, eqx, exact, against_oracle = CASES[case]
    cfg = _abi.default_config(**kw)
    refa, reads = streaming_input("mpm", eqx)
    g = grid_of(CELLS)
    with env(**dict(NO_SWITCH, PISCES_HIP_KERNEL=form, PISCES_HIP_READ_PATH=READ_PATHS[path])):
        with engine.HipVariantCaller(cfg) as c:
            if exact:
                c.SetIntervals(INTERVALS)
                c.SetExactTotalNumCalled(True)
            outs = []
            for when in ("before", "after"):
                if against_oracle:
                    outs.append(check(torch_cuda, g, cfg, form, caller=c, where="%s, %s the flushes" % (case, when)))
                else:
                    outs.append(run_fused(torch_cuda, c, view_of(torch_cuda, g)))
                if when == "before":
                    flush_in_every_form(c, refa, reads)
    (rows0, tr0), (rows1, tr1) = outs
    assert len(rows0) > 0 and rows1.tobytes() == rows0.tobytes() and tr1.tobytes() == tr0.tobytes()


def test_a_refused_flush_leaves_nothing_behind(torch_cuda):
    """NoiseModel.Window with an interval set and pisces_hip_set_exact_total_called: the flush is refused (PISCES_E_UNSUPPORTED) once its
    kernels are enqueued.  With the switch off again the same flush gives the rows, allele strings and Stats() of a handle that never
    made the refused call."""
    from pisces_amd import engine
    from pisces_amd._native import PiscesHipError
    refa, reads = streaming_input("mm")
    cfg = _abi.default_config(noise_model=1)
    out = []
    with env(**NO_SWITCH):
        for refused_first in (True, False):
            with engine.HipVariantCaller(cfg) as c:
                c.SetReference(refa)
                c.SetIntervals(INTERVALS[:2])
                c.AddAlleleCounts(_abi.ReadBatch(reads))
                if refused_first:
                    c.SetExactTotalNumCalled(True)
                    with pytest.raises(PiscesHipError) as refusal:
                        c.CallWithAlleles()
                    assert refusal.value.code == _abi.E_UNSUPPORTED
                    c.SetExactTotalNumCalled(False)
                rows, alleles = c.CallWithAlleles()
                out.append((rows.tobytes(), alleles, c.Stats()))
                assert len(rows) > 0 and c.Stats()["TotalNumCalled"] > 0
    assert out[0] == out[1]


def test_two_flushes_with_different_windows(torch_cuda):
    """MNV calling on, split form: the first batch has dirty loci, its tile kernels go first and leave a folded window; the second batch
    (reads that equal the reference) has neither.  The oracle's schedule, and the same run with PISCES_HIP_MNV_SPLIT=0."""
    from pisces_amd import engine
    from tests.test_gpu_parity import assert_records_match
    refa, reads = streaming_input("mp")
    cfg = _abi.default_config(call_mnvs=1)
    batch = _abi.ReadBatch(reads)
    exp, exp_alleles, exp_called = orc.run_reads_schedule(batch, refa, 1, len(refa), cfg, [1000])
    cats = (exp["info"] >> 4) & 7
    assert ((cats == _abi.CAT_MNV) & (exp["position"] <= 1000)).sum() >= 2 and (exp["position"] > 1000).sum() >= 500
    out = {}
    for split in (None, 0):
        with env(**dict(NO_SWITCH, PISCES_HIP_MNV_SPLIT=split)):
            with engine.HipVariantCaller(cfg) as c:
                c.SetReference(refa)
                c.AddAlleleCounts(batch)
                r1, a1 = c.CallWithAlleles(upToPosition=1000)
                r2, a2 = c.CallWithAlleles()
                out[split] = (np.concatenate([r1, r2]), a1 + a2, c.Stats())
        assert len(r1) and len(r2) and r1["position"].max() <= 1000 < r2["position"].min()
    rows, alleles, stats = out[None]
    assert alleles == exp_alleles
    assert_records_match(rows, exp)
    assert stats["TotalNumCalled"] == exp_called
    assert out[0][0].tobytes() == rows.tobytes() and out[0][1] == alleles and out[0][2] == stats
