"""The two VQR kernels on BASELINE config 2's rows ("VQR is IN").

BASELINE config 2's launch (100 000 loci x 500x) goes through pisces_hip_call_tiles + pisces_hip_compact_records; its compacted rows then
go through pisces_hip_vqr_count_device (edge checks on, extent 4) and pisces_hip_vqr_apply_device with a fixed pair of tables (C>T and G>A
in the basic and the edge table, every edge-risk rate 15: the synthetic SNVs have uniform alternate bases, so their own counts single
nothing out), one warm-up and REPS measured; the rows are restored from a copy before every repetition so that each update does the same
work.

    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/vqr_profile.py [REPS]      a run of its own
    python tools/vqr_profile.py --collect=TRACE [--out=DIR]   reads TRACE's kernel trace, drops the FIRST dispatch of the two VQR kernels (the
                                                              warm-up: code objects) and writes their statistics beside gather_direct_kernel's
                                                              (pisces_hip_compact_records over the same rows) to DIR/vqr_kernel_stats.csv; no GPU
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
COLLECT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--collect=")), None)
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def collect(trace_dir, out_dir):
    import csv
    per = {}
    for base, _, files in os.walk(trace_dir):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                for row in csv.DictReader(open(os.path.join(base, f))):
                    name = row["Kernel_Name"]
                    if "vqr_" in name or "gather_direct_kernel" in name:
                        per.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    assert any("vqr_" in k for k in per), "no VQR kernel in the trace under " + trace_dir
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "vqr_kernel_stats.csv")
    with open(path, "w", newline="") as fp:
        w = csv.writer(fp, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "DroppedFirstCalls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
        for name, spans in sorted(per.items()):
            drop = 1 if "vqr_" in name else 0
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
        d_sus = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros(34, dtype=torch.int64, device="cuda")
        d_changed = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.call_tiles(p.tuples.data_ptr(), p.tiles.data_ptr(), p.n_tiles, p.ref.data_ptr(), 1, p.ref_len, recs.data_ptr(), cap, tres.data_ptr(), ts)
    c.compact_records(recs.data_ptr(), tres.data_ptr(), p.n_tiles, offs.data_ptr(), out_d.data_ptr(), cap, count.data_ptr(), ts)
    c.synchronize()
    n = int(count.cpu()[0])
    with torch.cuda.stream(ts):
        keep = out_d.clone()
    opts = engine.vqr_options(do_amplicon_position_checks=1, extent_of_edge_region=4)
    tables = _abi.PiscesVqrTables()
    for cat in (5, 6):   # CtoT, GtoA
        tables.basic[cat] = tables.edge[cat] = 12
    tables.basic_mask = tables.edge_mask = (1 << 5) | (1 << 6)
    tables.edge_risk[:] = [15] * 12
    tables.has_edge_risk = 1
    for _ in range(1 + REPS):
        with torch.cuda.stream(ts):
            out_d.copy_(keep)
            d_counts.zero_()
            d_changed.zero_()
        c.vqr_count_device(out_d, cap, d_counts, opts, d_count=count, d_suspect=d_sus, stream=ts)
        c.vqr_apply_device(out_d, cap, tables, opts, d_count=count, d_suspect=d_sus, d_n_changed=d_changed, stream=ts)
        c.synchronize()
    v = d_counts.cpu().numpy()
    print(json.dumps({"workload": "BASELINE config 2 (100 000 loci x 500x) through call_tiles + compact_records", "rows": n, "row_bytes": 64 * n,
                      "reps": REPS, "snv_rows": int(v[:12].sum()), "rows_at_an_edge": int(v[33]), "suspects": int(v[17:33].sum()),
                      "rows_rewritten": int(d_changed.cpu()[0])}))
