"""BASELINE config 2's batch (100 000 loci x 500x, 333 500 reads) through the read store of a handle that tracks amplicon counts, every read
tagged with its synthetic amplicon's index: pisces_hip_add_device_reads_amplicons + pisces_hip_flush_view, a few times.  Run under
`rocprofv3 --kernel-trace --stats -- python tools/amplicon_profile.py` to read amplicon_tiles_kernel beside call_store_tiles_kernel."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pisces_amd import _abi, engine, synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
p = synth.make_pileup(n_loci=100_000, depth=500, device="cuda:0")
whole = synth.reads_of(p, p.base.shape[0], first_amplicon=p.first_amplicon)
ids = ((np.asarray(whole.position, dtype=np.int64) - (p.flank + 1)) // synth.READ_LEN).astype(np.int32)
d = engine.DeviceReadBatch.from_host(whole, "cuda:0")
d_ids = torch.as_tensor(ids, device="cuda:0")
with engine.HipVariantCaller(_abi.default_config()) as c:
    c.SetReference(p.ref.cpu().numpy())
    c.SetAmpliconBiasFilter(0.01)
    for _ in range(REPS):
        c.AddDeviceReads(d, amplicon_ids=d_ids)
        rows = c.CallView(None)
        n, flagged = len(rows), int(((rows["filter_bits"] >> 2) & 1).sum())
print(f"{whole.n_reads} reads, {len(np.unique(ids))} amplicons, {n} rows, {flagged} with AB, {REPS} flushes")
