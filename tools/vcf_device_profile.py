"""VCF body lines on the device against the host formatter on one core.

BASELINE config 2's launch (100 000 loci x 500x) goes through pisces_hip_call_tiles + pisces_hip_compact_records; its rows are then
formatted by pisces_hip_format_vcf_device (text in device memory, the size word in pinned host memory, one stream wait) and by
pisces_hip_format_vcf on the fetched rows.  Prints one JSON object: rows, bytes, the wall-clock pair (median / min / max of REPS), the
device span by HIP events, whether the two texts are equal, and the log10 sweep: SWEEP seeded strand-bias scores (uniform, log-uniform
down to 1e-10, and scores whose 10 log10 sits on a half of the fourth decimal) formatted on both sides, with the number of lines that
differ (expected 0; the first few are listed).

    python tools/vcf_device_profile.py [REPS] [SWEEP] [--out=DIR]     writes DIR/vcf_device.json (DIR defaults to profiles/) and prints it
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE -- python tools/vcf_device_profile.py --kernels
                                                                  a run of its own: one warm-up call, then REPS formatting calls
    python tools/vcf_device_profile.py --collect=TRACE [--out=DIR]   reads TRACE's kernel trace, drops the FIRST dispatch of every kernel
                                                                  (the warm-up call: code objects, scratch) and writes the statistics
                                                                  of the others to DIR/vcf_device_kernel_stats.csv; needs no GPU
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS_ONLY = "--kernels" in sys.argv
OUT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
COLLECT = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--collect=")), None)
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def collect(trace_dir, out_dir):
    """kernel_stats.csv's columns for this library's kernels from the per-dispatch trace, without the first dispatch of each kernel"""
    import csv
    per = {}
    for base, _, files in os.walk(trace_dir):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                for row in csv.DictReader(open(os.path.join(base, f))):
                    name = row["Kernel_Name"]
                    if "vcfdev::" in name or "pisces::" in name:
                        per.setdefault(name, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    assert per, "no kernel trace of this library under " + trace_dir
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "vcf_device_kernel_stats.csv")
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

REPS = int(args[0]) if len(args) > 0 else 5
SWEEP = int(args[1]) if len(args) > 1 else 10_000_000
CHUNK = 1_000_000


def config2_rows(c):
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
    return out_d, count, cap


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def sweep_scores(n, seed):
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 10, n)
    u = rng.random(n)
    s = np.where(kind < 5, u, 10.0 ** (-10.0 * u))
    j = rng.integers(0, 1_000_000, n)
    return np.where(kind >= 8, 10.0 ** (-(j + 0.5) * 1e-4 / 10.0), s)   # 10 log10 = -(j + 0.5)e-4: a half of the fourth decimal


with engine.HipVariantCaller(_abi.default_config()) as c:
    out_d, count, cap = config2_rows(c)
    n = int(count.cpu()[0])
    text = c.format_vcf_device("chr1", out_d, cap, d_count=count, capacity=160 * n)   # warm-up: scratch, code objects
    if KERNELS_ONLY:
        for _ in range(REPS):
            c.format_vcf_device("chr1", out_d, cap, d_count=count, capacity=160 * n)
        print(json.dumps({"rows": n, "text_bytes": len(text)}))
        sys.exit(0)
    rows = out_d.cpu().numpy().view(_abi.CALLED_ALLELE_DTYPE)[:n].copy()
    dev_ms, host_ms, span_ms = [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        text = c.format_vcf_device("chr1", out_d, cap, d_count=count, capacity=160 * n)
        dev_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host = engine.format_vcf("chr1", rows)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    # the three launches between two events, the text staying on the device
    ts = c.torch_stream()
    with torch.cuda.stream(ts):
        d_text = torch.empty(160 * n, dtype=torch.uint8, device="cuda")
        word = torch.zeros(1, dtype=torch.int64, device="cuda")
    cfg = _abi.PiscesVcfConfig()
    engine.lib.pisces_hip_vcf_default_config(cfg)
    for _ in range(REPS):
        c.mark(0, ts)
        engine.lib.pisces_hip_format_vcf_device(c._h, cfg, b"chr1", out_d.data_ptr(), cap, count.data_ptr(), None, None, None, None, d_text.data_ptr(),
                                                d_text.numel(), None, word.data_ptr(), ts.cuda_stream)
        c.mark(1, ts)
        span_ms.append(c.marked_ms())
    out = {"workload": "BASELINE config 2 (100 000 loci x 500x) through call_tiles + compact_records", "rows": n, "text_bytes": len(text),
           "bytes_per_line": len(text) / max(n, 1), "texts_equal": text == host.encode(), "reps": REPS,
           "device_wall_ms": spread(dev_ms), "host_one_core_wall_ms": spread(host_ms), "device_three_launches_ms": spread(span_ms),
           "host_us_per_line": float(np.median(host_ms)) * 1e3 / max(n, 1)}
    # config 4's row count (30 M): the same rows 300 times over, the three launches between two events, the text staying on the device
    big_n = 300 * n
    with torch.cuda.stream(ts):
        big = out_d[:n * 64].repeat(300)
        big_text = torch.empty(100 * big_n, dtype=torch.uint8, device="cuda")
    big_ms = []
    for k in range(4):   # the first call grows the handle's scratch and is not kept
        c.mark(0, ts)
        engine.lib.pisces_hip_format_vcf_device(c._h, cfg, b"chr1", big.data_ptr(), big_n, None, None, None, None, None, big_text.data_ptr(),
                                                big_text.numel(), None, word.data_ptr(), ts.cuda_stream)
        c.mark(1, ts)
        ms = c.marked_ms()
        if k:
            big_ms.append(ms)
    out["config4_scale"] = {"rows": big_n, "chunks": (big_n + 255) // 256, "text_bytes": int(word.cpu()[0]), "text_is_300_copies": int(word.cpu()[0]) == 300 * len(text),
                            "device_three_launches_ms": spread(big_ms)}
    del big, big_text
    # the log10 sweep
    base = np.zeros(CHUNK, dtype=_abi.CALLED_ALLELE_DTYPE)
    base["total_coverage"], base["allele_support"], base["reference_support"] = 1000, 100, 900
    base["info"] = 2 | (_abi.CAT_SNV << 4) | (0 << 7) | (3 << 10)
    differing, listed, done = 0, [], 0
    while done < SWEEP:
        k = min(CHUNK, SWEEP - done)
        r = base[:k].copy()
        r["position"] = np.arange(done + 1, done + k + 1)
        r["strand_bias_score"] = sweep_scores(k, 20261019 + done)
        with torch.cuda.stream(ts):
            d_r = torch.from_numpy(r.view(np.uint8).reshape(-1)).to("cuda")
        got = c.format_vcf_device("chr1", d_r, k).split(b"\n")
        want = engine.format_vcf("chr1", r).encode().split(b"\n")
        assert len(got) == len(want)
        for a, b, score in (() if got == want else zip(got, want, r["strand_bias_score"])):
            if a != b:
                differing += 1
                if len(listed) < 20:
                    listed.append({"score": float(score).hex(), "device": a.decode(), "host": b.decode()})
        done += k
    out["log10_sweep"] = {"scores": done, "differing_lines": differing, "first": listed}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vcf_device.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))
