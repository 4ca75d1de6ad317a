"""The three consensus kernels on BASELINE config 2's rows ("VennVcf is IN"): its 100 000 compacted rows are pool A, a copy
with seeded perturbed depths and PLANTED rows of disagreement pool B; one warm-up call and REPS measured.

    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/venn_profile.py [REPS]      a run of its own
    python tools/venn_profile.py --collect=TRACE [--out=DIR]   the kernels' statistics (first dispatch dropped) beside gather_direct_kernel's
                                                               over the same rows, to DIR/venn_kernel_stats.csv; no GPU
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
COLLECT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--collect=")), None)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
PLANTED = 4000


def collect(trace_dir, out_dir):
    import csv
    per = {}
    for base, _, files in os.walk(trace_dir):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                for row in csv.DictReader(open(os.path.join(base, f))):
                    name = row["Kernel_Name"]
                    if "venn_" in name or "gather_direct_kernel" in name:
                        per.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    assert any("venn_" in k for k in per), "no consensus kernel in the trace under " + trace_dir
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "venn_kernel_stats.csv")
    with open(path, "w", newline="") as fp:
        w = csv.writer(fp, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "DroppedFirstCalls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
        for name, spans in sorted(per.items()):
            drop = 1 if "venn_" in name else 0
            d = [b - a for a, b in sorted(spans)][drop:]
            if d:
                w.writerow([name, len(d), drop, int(sum(d)), float(np.mean(d)), int(min(d)), int(max(d)), float(np.std(d))])
    print(open(path).read())


if COLLECT:
    collect(COLLECT, OUT)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from pisces_amd import _abi, engine, synth  # noqa: E402

REPS = int(args[0]) if args else 5


def second_pool(rows, seed=20261020):
    """pool B from pool A's rows: every depth and support moved by a few per cent, PLANTED rows made to disagree"""
    rng = np.random.default_rng(seed)
    b = rows.copy()
    n = len(b)
    scale = rng.uniform(0.9, 1.1, n)
    for k in ("total_coverage", "allele_support", "reference_support"):
        b[k] = np.maximum(0, np.rint(b[k] * scale)).astype(np.int32)
    b["total_coverage"] = np.maximum(b["total_coverage"], b["allele_support"])
    cat = (b["info"] >> 4) & 7
    pick = rng.choice(n, size=min(PLANTED, n), replace=False)
    for i in pick:
        word = int(b["info"][i])
        ref = (word >> 7) & 7
        if cat[i] == _abi.CAT_REFERENCE:   # a 5 % SNV where pool A has the reference
            alt = (ref + 1 + int(rng.integers(3))) % 4
            b["allele_support"][i] = b["total_coverage"][i] // 20
            b["reference_support"][i] = b["total_coverage"][i] - b["allele_support"][i]
            b["info"][i] = (word & ~0x1FFF) | _abi.GT_HET_ALT_REF | (_abi.CAT_SNV << 4) | (ref << 7) | (alt << 10)
        else:                                # another alternate
            alt = (word >> 10) & 7
            b["info"][i] = (word & ~(7 << 10)) | ((((alt if alt < 4 else 0) + 1) % 4) << 10)
    return b


with engine.HipVariantCaller(_abi.default_config()) as c:
    p = synth.make_pileup(n_loci=100_000, depth=500, device="cuda")
    cap = p.n_tiles * _abi.SLOTS_PER_TILE
    ts = c.torch_stream()
    with torch.cuda.stream(ts):
        recs = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
        tres = torch.zeros(p.n_tiles * _abi.TILE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        out_d = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
        offs = torch.zeros(p.n_tiles, dtype=torch.int32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    c.call_tiles(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, recs.data_ptr(), cap, tres.data_ptr(), ts)
    c.compact_records(recs.data_ptr(), tres.data_ptr(), p.n_tiles, offs.data_ptr(), out_d.data_ptr(), cap, count.data_ptr(), ts)
    c.synchronize()
    n = int(count.cpu()[0])
    rows_a = out_d.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy()
    rows_b = second_pool(rows_a)
    with torch.cuda.stream(ts):
        d_b = torch.from_numpy(rows_b.view(np.uint8).reshape(-1).copy()).to("cuda")
        d_rows = torch.zeros(2 * n * 64, dtype=torch.uint8, device="cuda")
        d_idx = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        d_info = torch.zeros(2 * n * 32, dtype=torch.uint8, device="cuda")
        d_venn_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_venn_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_n_out = torch.zeros(3, dtype=torch.int64, device="cuda")
    opts = engine.venn_options()
    a, b = engine.venn_rows(out_d, cap, count), engine.venn_rows(d_b, n)
    out = engine.venn_out(d_rows, d_idx, None, None, d_n_out, 2 * n, 0, 0, info=d_info, venn_a=d_venn_a, venn_b=d_venn_b)
    for _ in range(1 + REPS):
        c.venn_consensus_device(a, b, out, opts, stream=ts)
        c.synchronize()
    rows_out = int(d_n_out.cpu()[0])
    host = engine.venn_consensus(rows_a, rows_b, opts)
    assert host["n_out"][0] == rows_out and d_rows.cpu().numpy()[:rows_out * 64].tobytes() == host["records"].tobytes()
    cases = np.bincount(host["info"]["comparison_case"], minlength=4)
    moved = 64 * (2 * n + rows_out) + 32 * rows_out + 4 * rows_out + 2 * n
    print(json.dumps({"workload": "BASELINE config 2 (100 000 loci x 500x) through call_tiles + compact_records, a perturbed copy as pool B", "rows_a": n, "rows_b": n,
                      "planted": PLANTED, "rows_out": rows_out, "reps": REPS, "cases": {"agreed_on_reference": int(cases[0]), "agreed_on_alternate": int(cases[1]),
                      "one_reference_one_alternate": int(cases[2]), "can_not_combine": int(cases[3])}, "pool_bias_rows": int(((host["records"]["filter_bits"] >> 1) & 1).sum()),
                      "bytes_the_emit_kernel_moves": moved, "device_equals_host_entry": True}))
