"""Scylla's read pass (pisces_hip_vead_groups_device, DESIGN section 7, "Scylla's read pass is IN") on a config-3-like batch: synth.mixed_reads
at depth DEPTH over N_LOCI loci (SNVs, MNVs, deletions and insertions planted in the reads), handed over in device memory; neighbourhoods
of 2-40 SNV / insertion / deletion sites within 50 bases planted every EVERY bases.  One warm-up call and REPS measured; the wall time of a
call up to its outputs (the call's one wait included), and, for comparison, the wall time of this library's own host loop
(pisces_hip_vead_groups, one core) over the same input: that is NOT the reference, whose C# does not run here.  Prints one JSON line with
the shapes and the bytes each kernel must move, derived from them.

    python tools/vead_profile.py [N_LOCI] [REPS] [--no-host]
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/vead_profile.py [N_LOCI] [REPS] --no-host     a run of its own
    python tools/vead_profile.py --collect=TRACE [--out=DIR]   the kernels' statistics (first dispatch dropped) to DIR/vead_kernel_stats.csv; no GPU
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
                    if "vead_" in row["Kernel_Name"]:
                        per.setdefault(row["Kernel_Name"], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    assert per, "no vead kernel in the trace under " + trace_dir
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "vead_kernel_stats.csv")
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

N_LOCI = int(args[0]) if args else 30_000
REPS = int(args[1]) if len(args) > 1 else 5
DEPTH, SEED, EVERY = 2000, 33, 300

n_loci = (N_LOCI // synth.READ_LEN) * synth.READ_LEN
p = synth.make_pileup(n_loci, DEPTH, seed=SEED, device="cuda", first_locus=0, total_loci=n_loci, with_tuples=False)
batch, planted = synth.mixed_reads(p, SEED)
d = engine.DeviceReadBatch.from_host(batch, "cuda:0")
d.synchronize()

rng = np.random.default_rng(SEED)
first, last = int(batch.position[0]), int(batch.position[-1]) + synth.READ_LEN
rows, nbhd = [], []
for start in range(first + 20, last - 60, EVERY):
    n = int(rng.integers(2, 41))
    begin = len(rows)
    for pos in np.sort(rng.integers(start, start + 50, n)):
        kind, b = rng.integers(0, 4), "ACGT"[int(rng.integers(0, 4))]
        alt = "ACGT"[int(rng.integers(0, 4))]
        rows.append((int(pos), b, alt) if kind < 2 else (int(pos), b, b + "AC"[:int(rng.integers(1, 3))]) if kind == 2 else (int(pos), b + "GT"[:int(rng.integers(1, 3))], b))
    nbhd.append((begin, len(rows)))
sites = engine.vead_sites(rows)

dev = torch.device("cuda", 0)
with engine.HipVariantCaller(_abi.default_config()) as c:
    def call(caps):
        with torch.cuda.stream(c.torch_stream()):
            groups = torch.empty(max(caps[0], 1) * 24, dtype=torch.uint8, device=dev)
            states = torch.empty(max(caps[1], 1), dtype=torch.uint8, device=dev)
            info = torch.empty(len(nbhd) * 32, dtype=torch.uint8, device=dev)
            n_out = torch.zeros(3, dtype=torch.int64, device=dev)
        c.synchronize()
        t0 = time.perf_counter()
        c.vead_groups_device(sites, nbhd, engine.vead_out(groups, states, info, n_out, caps[0], caps[1]), batch=d)
        c.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, [int(v) for v in n_out.cpu()], info.cpu().numpy().view(_abi.VEAD_INFO_DTYPE)

    _, counts, _ = call((0, 0))                  # warm-up: the counts, the scratch
    walls = []
    for _ in range(REPS):
        ms, again, info = call((counts[0], counts[1]))
        assert again == counts
        walls.append(ms)

pairs = int(info["n_reads_used"].sum())          # (the pairs a neighbourhood's range holds are these plus the skipped and the stopping read)
words = sum(-(-(e - b) // 32) for b, e in nbhd)
out = {"loci": n_loci, "depth": DEPTH, "reads": int(batch.n_reads), "cigar_ops": int(len(batch.cigar_op)), "bases": int(len(batch.bases)),
       "neighbourhoods": len(nbhd), "sites": len(rows), "reads_used_pairs": pairs, "groups": counts[0], "state_bytes": counts[1], "reps": REPS,
       "device_call_wall_ms": {"median": float(np.median(walls)), "min": min(walls), "max": max(walls)}}
# what each kernel must move, from the shapes (bytes)
nr, no = int(batch.n_reads), int(len(batch.cigar_op))
mean_read = len(batch.bases) / max(nr, 1)
out["bytes"] = {
    "vead_spans_kernel": nr * (4 + 8 + 4 + 1) + no * 5,                        # position, two offsets, end, flags out; the CIGAR
    "vead_ranges_kernel": len(nbhd) * (16 + 8) + len(nbhd) * 2 * 4 * int(np.ceil(np.log2(max(nr, 2)))),
    "vead_states_kernel": int(pairs * (9 + 8 + 2 * mean_read + 5 * no / max(nr, 1)) + pairs * 8 * words / max(len(nbhd), 1)),   # a read's arrays, its key
    "vead_group_kernel": int(pairs * (1 + 2 * 8 * words / max(len(nbhd), 1) + 8)),   # flag, own key and the occupant's, a slot and its count
    "vead_mark_kernel": int(2 * pairs * 8),                                     # two slots a pair, table and count
    "vead_count_kernel": int(pairs * 4 + pairs / 64 * 4),
    "vead_scan_kernel": int(pairs / 64 * (8 + 4 + 16)),
    "vead_emit_kernel": int(pairs * 4 + counts[0] * (24 + 16) + 2 * counts[1]),
    "vead_info_kernel": len(nbhd) * (48 + 16 + 32 + 8 + 32),
}
if "--no-host" not in sys.argv:
    t0 = time.perf_counter()
    host = engine.vead_groups(batch, sites, nbhd, capacities=(counts[0], counts[1]))
    out["host_loop_one_core_ms"] = (time.perf_counter() - t0) * 1e3
    out["host_loop_note"] = "pisces_hip_vead_groups of this library on one core, one call with the right capacities; not the reference"
    assert host["n_out"][:2] == (counts[0], counts[1])
print(json.dumps(out))
