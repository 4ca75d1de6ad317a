"""CoverageMethod.Exact against Approximate on one build: a config-3-like mix (synth.mixed_reads: SNVs, MNVs of 2-3 bases, deletions of 1-10,
insertions of 1-6; MNV calling on, -maxmnvlength 3 -maxgapbetweenmnv 1) at BASELINE config 3's depth (2000x) over N_LOCI loci, reads handed
over in device memory, one flush.  Alternates an exact and an Approximate handle REPS times and prints, per handle kind, the flush's device
time by HIP events (pisces_hip_set_chain_timing: first kernel of the flush to its compacted records), its wall time on the host, the
spread and the ratio; and the bytes exact_span_kernel reads, from the shapes (16 B summary + 16 B descriptor of every read in a
candidate's search range is an upper bound: 32 B x reads of the segment x spanning candidates; the CIGAR and per-base directions of
multi-direction reads come on top).

    python tools/exact_profile.py [N_LOCI] [REPS]
    rocprofv3 --kernel-trace --stats -- python tools/exact_profile.py          exact_span_kernel and exact_summary_kernel beside
                                                                                call_spanning_kernel and call_store_tiles_kernel
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pisces_amd import _abi, engine, synth  # noqa: E402

N_LOCI = int(sys.argv[1]) if len(sys.argv) > 1 else 30_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
DEPTH, SEED = 2000, 33

n_amp = N_LOCI // synth.READ_LEN
n_loci = n_amp * synth.READ_LEN
ref = synth.reference_of(n_loci, SEED, device="cuda")
p = synth.make_pileup(n_loci, DEPTH, seed=SEED, device="cuda", first_locus=0, total_loci=n_loci, with_tuples=False)
batch, planted = synth.mixed_reads(p, SEED)
d = engine.DeviceReadBatch.from_host(batch, "cuda:0")
cfg = _abi.default_config(call_mnvs=1, max_mnv_length=3, max_gap_between_mnv=1)


def one(exact):
    with engine.HipVariantCaller(cfg) as c:
        c.SetReference(ref)
        if exact:
            c.SetCoverageMethod("exact")
        c.SetChainTiming(True)
        c.AddDeviceReads(d)
        c.synchronize()
        t0 = time.perf_counter()
        rows = c.CallView(None)
        wall = (time.perf_counter() - t0) * 1e3
        add_ms, flush_ms = c.ChainTime()
        cat = (rows["info"] >> 4) & 7
        spanning = int(np.isin(cat, (_abi.CAT_INSERTION, _abi.CAT_DELETION, _abi.CAT_MNV)).sum())
        return {"add_device_ms": add_ms, "flush_device_ms": flush_ms, "flush_wall_ms": wall, "rows": len(rows), "spanning_rows": spanning}


one(False)   # warm-up: memo tables, allocations
runs = {"exact": [], "approximate": []}
for _ in range(REPS):
    runs["exact"].append(one(True))
    runs["approximate"].append(one(False))
out = {"loci": n_loci, "depth": DEPTH, "reads": batch.n_reads, "planted": len(planted), "reps": REPS, "runs": runs}
for kind, rs in runs.items():
    for key in ("flush_device_ms", "flush_wall_ms", "add_device_ms"):
        v = [r[key] for r in rs]
        out[f"{kind}_{key}"] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
out["flush_wall_ratio_exact_over_approximate"] = out["exact_flush_wall_ms"]["median"] / out["approximate_flush_wall_ms"]["median"]
out["span_kernel_bytes_upper_bound"] = 32 * batch.n_reads * runs["exact"][0]["spanning_rows"]
print(json.dumps(out))
