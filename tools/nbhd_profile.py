"""Scylla's neighbourhoods (pisces_hip_nbhd_build_device, DESIGN section 7, "Scylla's neighbourhoods are IN") on BASELINE config 2's rows.

BASELINE config 2's launch (100 000 loci x 500x) goes through pisces_hip_call_tiles + pisces_hip_compact_records; of its compacted rows
one every 20 to 40 (seeded, about every 30 bases) is made a passing 0/1 SNV row, every tenth of those with a co-located second allele and
every twentieth with a LowVariantQscore bit; everything else is a Reference row.  The rows stay on the device.  One warm-up call (the
counts, the scratch) and REPS measured calls into device buffers of the right sizes: the wall time of a call up to its outputs, and, for
scale, this library's own host entry (pisces_hip_nbhd_build, one core) over the same rows: that is NOT the reference, whose C# does not
run here.  Prints one JSON line.

    python tools/nbhd_profile.py [REPS] [--no-host]
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/nbhd_profile.py [REPS] --no-host     a run of its own
    python tools/nbhd_profile.py --collect=TRACE [--out=DIR]   the kernels' statistics (first dispatch dropped) to DIR/nbhd_kernel_stats.csv; no GPU
"""
import json
import os
import sys
import time

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
                    if "nbhd_" in row["Kernel_Name"]:
                        per.setdefault(row["Kernel_Name"], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    assert per, "no nbhd kernel in the trace under " + trace_dir
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "nbhd_kernel_stats.csv")
    with open(path, "w", newline="") as fp:
        w = csv.writer(fp, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "DroppedFirstCalls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "StdDev"])
        for name, spans in sorted(per.items()):
            d = [b - a for a, b in sorted(spans)][1:]
            if d:
                w.writerow([name, len(d), 1, int(sum(d)), float(np.mean(d)), int(min(d)), int(max(d)), float(np.std(d))])
    print(open(path).read())


if COLLECT:
    collect(COLLECT, OUT)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from pisces_amd import _abi, engine, synth  # noqa: E402

REPS = int(args[0]) if args else 5
SEED = 41
ITEM = {"sites": 16, "alleles": 1, "site_row": 4, "site_original": 4, "neighbourhoods": 8, "info": 48, "ref_bytes": 1}
CAPACITY_OF = {"neighbourhoods": 0, "info": 0, "sites": 1, "site_row": 1, "site_original": 1, "alleles": 2, "ref_bytes": 3}

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

    # the seeded variants, planted in a host copy of the rows (set-up, not measured)
    rows = out_d.cpu().numpy()[:n * 64].view(_abi.CALLED_ALLELE_DTYPE).copy()
    rows = rows[np.argsort(rows["position"], kind="stable")]
    _, first_of_position = np.unique(rows["position"], return_index=True)
    rows = rows[first_of_position]                                  # one row a position ...
    rng = np.random.default_rng(SEED)
    ref_code = (rows["info"] >> 7) & 7
    rows["info"] = _abi.GT_HOM_REF | (_abi.CAT_REFERENCE << 4) | (ref_code << 7) | (ref_code << 10)   # ... every one a Reference row
    rows["filter_bits"] = 0
    at, planted, k = int(rng.integers(0, 30)), [], 0
    while at < len(rows):
        planted.append(at)
        at += int(rng.integers(20, 41))
    extra = []
    for k, r in enumerate(planted):
        code = int(ref_code[r]) & 3
        rows["info"][r] = _abi.GT_HET_ALT_REF | (_abi.CAT_SNV << 4) | (code << 7) | (((code + 1) & 3) << 10)
        if k % 20 == 7:
            rows["filter_bits"][r] = 1 << _abi.FILTER_LOW_VARIANT_QSCORE
        if k % 10 == 3:
            second = rows[r].copy()
            second["info"] = _abi.GT_HET_ALT_REF | (_abi.CAT_SNV << 4) | (code << 7) | (((code + 2) & 3) << 10)
            extra.append(second)
    if extra:
        rows = np.concatenate([rows, np.array(extra, dtype=rows.dtype)])
        rows = rows[np.argsort(rows["position"], kind="stable")]
    n = len(rows)
    dev = torch.device("cuda", c.device)
    with torch.cuda.stream(ts):
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
    c.synchronize()
    venn_rows = engine.venn_rows(d_rows, n)
    criteria = engine.nbhd_criteria(passing_variants_only=0)

    def call(caps):
        with torch.cuda.stream(ts):
            t = {k: torch.empty(max(caps[CAPACITY_OF[k]] * ITEM[k], 1), dtype=torch.uint8, device=dev) for k in ITEM}
            t["row_class"] = torch.empty(n, dtype=torch.uint8, device=dev)
            n_out = torch.zeros(6, dtype=torch.int64, device=dev)
        out = engine.nbhd_out(t["sites"], t["alleles"], t["site_row"], t["site_original"], t["neighbourhoods"], t["info"], t["ref_bytes"], n_out, *caps,
                              row_class=t["row_class"])
        c.synchronize()
        t0 = time.perf_counter()
        c.nbhd_build_device(venn_rows, out, criteria)
        c.synchronize()
        return (time.perf_counter() - t0) * 1e3, [int(v) for v in n_out.cpu()]

    _, counts = call((0, 0, 0, 0))               # warm-up: the counts, the scratch
    walls = []
    for _ in range(REPS):
        ms, again = call(tuple(counts[:4]))
        assert again == counts
        walls.append(ms)

out = {"workload": "BASELINE config 2 (100 000 loci x 500x) through call_tiles + compact_records, one row a position, seeded SNV rows every 20-40 rows",
       "rows": n, "row_bytes": 64 * n, "planted": len(planted) + len(extra), "kept_neighbourhoods": counts[0], "sites": counts[1], "allele_bytes": counts[2],
       "reference_bytes": counts[3], "raw_neighbourhoods": counts[4], "eligible_rows": counts[5], "reps": REPS,
       "device_call_wall_ms": {"median": float(np.median(walls)), "min": min(walls), "max": max(walls)}}
if "--no-host" not in sys.argv:
    t0 = time.perf_counter()
    host = engine.nbhd_build(rows, None, criteria, capacities=tuple(counts[:4]))
    out["host_entry_one_core_ms"] = (time.perf_counter() - t0) * 1e3
    out["host_entry_note"] = "pisces_hip_nbhd_build of this library on one core, one call with the right capacities; not the reference"
    assert list(host["n_out"]) == counts
print(json.dumps(out))
