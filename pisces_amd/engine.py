"""Host-side mirror of the reference's operator surface for the hot path, over the C ABI.

`HipVariantCaller` plays the three objects Factory.CreateSomaticVariantCaller builds
(src/exe/Pisces/Logic/Factory.cs:253-269): ICandidateVariantFinder + IStateManager
(AddAlleleCounts / GetAlleleCount / GetCandidatesToProcess / DoneProcessing) + IAlleleCaller.Call,
with the reference's method names so the parity tests read like the reference's own tests.
Every compute call goes through libpisceship.so (HIP); nothing here has a CPU path.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._native import PiscesHipError, lib


def _check(handle, rc):
    if rc != 0:
        msg = lib.pisces_hip_last_error(handle)
        raise PiscesHipError(rc, msg.decode() if msg else "")


class DeviceReadBatch:
    """A PiscesReadBatch whose arrays are torch tensors in device memory (what pisces_hip_add_device_reads takes): position / cigar_offset /
    seq_offset int32, flags / cigar_op / bases / quals (/ directions / deletion_directions) uint8, cigar_len int32 holding the uint32 bits."""

    def __init__(self, position, flags, cigar_offset, cigar_op, cigar_len, seq_offset, bases, quals, directions=None, deletion_directions=None,
                 n_ops=None, n_bases=None):
        import torch
        self.torch = torch
        self.tensors = dict(position=position, flags=flags, cigar_offset=cigar_offset, cigar_op=cigar_op, cigar_len=cigar_len, seq_offset=seq_offset,
                            bases=bases, quals=quals, directions=directions, deletion_directions=deletion_directions)
        for k, t in self.tensors.items():
            assert t is None or (t.is_cuda and t.is_contiguous()), k
        self.n_reads = int(position.numel())
        self.n_ops = int(cigar_op.numel()) if n_ops is None else int(n_ops)
        self.n_bases = int(bases.numel()) if n_bases is None else int(n_bases)
        c = _abi.PiscesReadBatch()
        c.n_reads = self.n_reads
        for k, t in self.tensors.items():
            setattr(c, k, C.cast(C.c_void_p(t.data_ptr() if t is not None else 0), type(getattr(c, k))))
        self.c = c

    @classmethod
    def from_host(cls, batch, device="cuda:0"):
        import torch
        up = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to(device)
        # (an empty tensor has no storage to point at: one spare element keeps every pointer valid)
        pad = lambda t: t if t is None or t.numel() else torch.zeros(1, dtype=t.dtype, device=device)
        return cls(pad(up(batch.position)), pad(up(batch.flags)), pad(up(batch.cigar_offset)), pad(up(batch.cigar_op)), pad(up(batch.cigar_len, np.int32)),
                   pad(up(batch.seq_offset)), pad(up(batch.bases)), pad(up(batch.quals)), pad(up(batch.directions)),
                   pad(up(getattr(batch, "deletion_directions", None))), n_ops=len(batch.cigar_op), n_bases=len(batch.bases))

    def synchronize(self):
        self.torch.cuda.synchronize(self.tensors["position"].device)


class _RowsAt:
    """memory of the library (the pinned download buffer) shown to numpy without a copy"""
    __slots__ = ("__array_interface__",)


class HipVariantCaller:
    def __init__(self, config=None, device=0):
        self.config = config if config is not None else _abi.default_config()
        h = C.c_void_p()
        rc = lib.pisces_hip_create(C.byref(self.config), device, C.byref(h))
        if rc != 0:
            raise PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode())
        self._h = h
        self.device = device

    # ---- lifetime (C# IDisposable) ----
    def close(self):
        if getattr(self, "_h", None):
            self._torch_stream = None   # (an ExternalStream over the handle's stream: dead with the handle)
            lib.pisces_hip_destroy(self._h)
            self._h = None

    Dispose = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    # ---- ChrReference ----
    def SetReference(self, sequence):
        """ChrReference.Sequence (upper case). position p is sequence[p-1]."""
        if isinstance(sequence, str):
            sequence = sequence.encode()
        arr = np.frombuffer(bytes(sequence), dtype=np.uint8) if not isinstance(sequence, np.ndarray) else \
            np.ascontiguousarray(sequence, np.uint8)
        _check(self._h, lib.pisces_hip_set_reference(self._h, arr.ctypes.data, arr.size))

    def SetIntervals(self, intervals):
        """ChrIntervalSet (sorted, disjoint, inclusive)."""
        iv = np.asarray(intervals, dtype=np.int32).reshape(-1, 2)   # (pairs, or an (n, 2) array: 16 000 tuples taken apart in Python were 2 ms a call)
        s, e = np.ascontiguousarray(iv[:, 0]), np.ascontiguousarray(iv[:, 1])
        _check(self._h, lib.pisces_hip_set_intervals(self._h, s.ctypes.data, e.ctypes.data, len(s)))

    def SetOwnedRange(self, lo, hi):
        """pisces_hip_set_owned_range: the positions this shard owns (candidates of its halo reads outside them are the neighbour's)."""
        _check(self._h, lib.pisces_hip_set_owned_range(self._h, int(lo), int(hi)))

    def SetCoverageMethod(self, method):
        """PiscesApplicationOptions.CoverageMethod: "approximate" / "exact" (or _abi.COVERAGE_*), before the first read is added.  An exact
        handle counts the reads that span every insertion, deletion and MNV of a flush (ExactCoverageCalculator) from the read store."""
        if isinstance(method, str):
            names = {"approximate": _abi.COVERAGE_APPROXIMATE, "exact": _abi.COVERAGE_EXACT}
            if method.lower() not in names:
                raise PiscesHipError(_abi.E_INVALID_ARG, f"SetCoverageMethod: {method!r} is no CoverageMethod")
            method = names[method.lower()]
        _check(self._h, lib.pisces_hip_set_coverage_method(self._h, int(method)))

    set_coverage_method = SetCoverageMethod

    def SetIndelRepeatFilter(self, threshold):
        """VariantCallingParameters.IndelRepeatFilter (-RepeatFilter_ToBeRetired): above 0, every flush gives the insertion and deletion rows
        whose repeat length (indel_repeat_length) reaches it FILTER_INDEL_REPEAT_LENGTH; 0 = off, the default.  Any time; from the next flush.
        Give format_vcf / format_vcf_device indel_repeat_filter=threshold to have the bit printed as R<threshold>."""
        _check(self._h, lib.pisces_hip_set_indel_repeat_filter(self._h, int(threshold)))

    def GetSpanningReadCounts(self, preceding, trailing, is_insertion=False):
        """What ExactCoverageCalculator needs of IAlleleSource.GetSpanningReadSummaries(preceding, trailing): the reads the store holds that
        span the two positions, by direction (int32[3]).  An exact handle only."""
        out = (C.c_int32 * 3)()
        _check(self._h, lib.pisces_hip_get_spanning_read_counts(self._h, int(preceding), int(trailing), int(bool(is_insertion)), out))
        return np.array(list(out), dtype=np.int32)

    spanning_read_counts = GetSpanningReadCounts

    # ---- IStateManager ----
    def SetAmpliconBiasFilter(self, threshold):
        """VariantCallingParameters.AmpliconBiasFilterThreshold (None = off): before the first read is added."""
        _check(self._h, lib.pisces_hip_set_amplicon_bias_filter(self._h, -1.0 if threshold is None else float(threshold)))

    def AddAlleleCounts(self, reads, amplicon_ids=None):
        """IStateManager.AddAlleleCounts for a batch (one _abi.ReadBatch, or an iterable of read dicts); amplicon_ids: one int32 per read
        (Read.GetAmpliconNameIfExists as an id of the host's choosing, -1 = no tag)."""
        batch = reads if isinstance(reads, _abi.ReadBatch) else _abi.ReadBatch(reads)
        if amplicon_ids is None:
            _check(self._h, lib.pisces_hip_add_reads(self._h, C.byref(batch.c)))
            return
        ids = np.ascontiguousarray(amplicon_ids, dtype=np.int32)
        if ids.shape != (batch.c.n_reads,):
            raise PiscesHipError(_abi.E_INVALID_ARG, "AddAlleleCounts: one amplicon id per read")
        _check(self._h, lib.pisces_hip_add_reads_amplicons(self._h, C.byref(batch.c), ids.ctypes.data))

    def GetCoverageByAmplicon(self, position, n=1):
        """IAlleleSource.GetCoverageByAmplicon for n positions from `position` on: (ids[n][6], coverage[n][6], support[n][4][6] by base A C G T),
        slots in ascending id order, -1 / 0 in the unused ones."""
        ids = np.full((n, 6), -1, dtype=np.int32)
        cov = np.zeros((n, 6), dtype=np.int32)
        sup = np.zeros((n, 4, 6), dtype=np.int32)
        _check(self._h, lib.pisces_hip_get_amplicon_counts(self._h, int(position), int(n), ids.ctypes.data, cov.ctypes.data, sup.ctypes.data))
        return ids, cov, sup

    def AddDeviceReads(self, reads, amplicon_ids=None):
        """pisces_hip_add_device_reads: IStateManager.AddAlleleCounts for a batch that lies in device memory.  `reads`: a DeviceReadBatch
        (torch tensors on the handle's device), or an _abi.ReadBatch whose arrays are copied there first (test plumbing).  The library
        has read the last byte of the tensors when the call returns (pisces_hip.h): the caller may overwrite or free them at once, on any
        stream — which is what lets the temporaries of the second form go back to torch's allocator here."""
        b = reads if isinstance(reads, DeviceReadBatch) else DeviceReadBatch.from_host(reads if isinstance(reads, _abi.ReadBatch) else _abi.ReadBatch(reads),
                                                                                       f"cuda:{self.device}")
        b.synchronize()
        if amplicon_ids is not None:
            import torch
            ids = amplicon_ids if isinstance(amplicon_ids, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(amplicon_ids, dtype=np.int32), device=f"cuda:{self.device}")
            if ids.dtype != torch.int32 or ids.numel() != b.c.n_reads or not ids.is_cuda:
                raise PiscesHipError(_abi.E_INVALID_ARG, "AddDeviceReads: one int32 amplicon id per read, on the device")
            torch.cuda.synchronize(ids.device)
            _check(self._h, lib.pisces_hip_add_device_reads_amplicons(self._h, C.byref(b.c), b.n_ops, b.n_bases, ids.data_ptr()))
            return
        _check(self._h, lib.pisces_hip_add_device_reads(self._h, C.byref(b.c), b.n_ops, b.n_bases))

    def StageReads(self, reads):
        """pisces_hip_stage_reads: the arrays of `reads` (an _abi.ReadBatch) written into the handle's pinned staging buffer, as a host
        that marshals its reads straight into it would leave them; returns the batch to hand to AddAlleleCounts (valid until the next
        call on the handle that is not that AddAlleleCounts)."""
        b = reads if isinstance(reads, _abi.ReadBatch) else _abi.ReadBatch(reads)
        views = _abi.PiscesReadBatch()
        dd = getattr(b, "deletion_directions", None)
        _check(self._h, lib.pisces_hip_stage_reads(self._h, b.n_reads, len(b.cigar_op), b.n_bases, 1 if b.directions is not None else 0,
                                                   1 if dd is not None else 0, C.byref(views)))

        def fill(ptr, arr):
            if arr is not None and arr.size:
                C.memmove(ptr, arr.ctypes.data, arr.nbytes)

        fill(views.position, b.position); fill(views.flags, b.flags); fill(views.cigar_offset, b.cigar_offset)
        fill(views.cigar_op, b.cigar_op); fill(views.cigar_len, b.cigar_len); fill(views.seq_offset, b.seq_offset)
        fill(views.bases, b.bases); fill(views.quals, b.quals); fill(views.directions, b.directions); fill(views.deletion_directions, dd)
        staged = _abi.ReadBatch.__new__(_abi.ReadBatch)
        staged.c = views
        staged.n_reads = b.n_reads
        staged.n_bases = b.n_bases
        return staged

    def AddObservations(self, positions, tuples):
        positions = np.ascontiguousarray(positions, np.int32)
        tuples = np.ascontiguousarray(tuples, np.uint32)
        assert positions.shape == tuples.shape
        _check(self._h, lib.pisces_hip_add_observations(self._h, positions.ctypes.data, tuples.ctypes.data, positions.size))

    def GetCounts(self, start_position, n):
        out = np.zeros((n, 6, 3, _abi.NUM_ANCHORS), dtype=np.int32)
        _check(self._h, lib.pisces_hip_get_counts(self._h, start_position, n, out.ctypes.data))
        return out

    def GetBaseQualitySums(self, start_position, n):
        """RegionState._sumOfAlleleBaseQualities of [start_position, start_position + n): double[n][6][3][11]."""
        out = np.zeros((n, 6, 3, _abi.NUM_ANCHORS), dtype=np.float64)
        _check(self._h, lib.pisces_hip_get_base_quality_sums(self._h, int(start_position), int(n), out.ctypes.data))
        return out

    def GetGappedMnvRefCount(self, position):
        v = C.c_int32(0)
        _check(self._h, lib.pisces_hip_get_gapped_mnv_ref(self._h, int(position), C.byref(v)))
        return int(v.value)

    def GetAlleleCount(self, position, allele_type, direction_type, minAnchor=0, maxAnchor=None, fromEnd=False,
                       symmetric=False):
        """IAlleleSource.GetAlleleCount (src/lib/Pisces.Domain/Interfaces/IAlleleSource.cs): the anchor window
        arithmetic is AlleleCountHelper.GetAnchorAdjustedAlleleCount (AlleleCountHelper.cs:21-85) applied to
        the device-served counts."""
        if position <= 0:
            raise PiscesHipError(_abi.E_INVALID_ARG, "Position must be greater than 0.")
        c = self.GetCounts(position, 1)[0, allele_type, direction_type]
        return anchor_adjusted_count(c, minAnchor, maxAnchor, fromEnd, symmetric)

    def AddGappedMnvRefCount(self, support_lookup):
        pos = np.array(list(support_lookup.keys()), dtype=np.int32)
        cnt = np.array(list(support_lookup.values()), dtype=np.int32)
        _check(self._h, lib.pisces_hip_add_gapped_mnv_ref(self._h, pos.ctypes.data, cnt.ctypes.data, len(pos)))

    # ---- GetCandidatesToProcess + IAlleleCaller.Call + DoneProcessing ----
    def Call(self, upToPosition=None, capacity=1 << 16, reuse_buffer=False):
        """SmallVariantCaller.Call(upToPosition) (SmallVariantCaller.cs:157-189). None = final flush.
        Returns a CALLED_ALLELE_DTYPE array sorted by (position, ref, alt).  reuse_buffer: the rows are a view into a buffer the engine
        keeps from call to call (valid until the next Call), as a host that owns its output buffer works; the default hands
        out a fresh array every time."""
        up_to = -1 if upToPosition is None else int(upToPosition)
        while True:
            if reuse_buffer:
                out = getattr(self, "_flush_out", None)
                if out is None or len(out) < capacity:
                    out = self._flush_out = np.zeros(capacity, dtype=_abi.CALLED_ALLELE_DTYPE)
            else:
                out = np.zeros(capacity, dtype=_abi.CALLED_ALLELE_DTYPE)
            n = C.c_int64(0)
            rc = lib.pisces_hip_flush(self._h, up_to, out.ctypes.data, len(out), C.byref(n))
            if rc == _abi.E_BUFFER_TOO_SMALL:
                capacity = int(n.value)
                continue
            _check(self._h, rc)
            return out[: n.value]

    def CallView(self, upToPosition=None):
        """pisces_hip_flush_view: Call() whose rows are NOT copied — the array aliases memory of the handle (the pinned buffer the device
        wrote the records to) and is valid until the next Call* on this caller."""
        rows, n = C.c_void_p(), C.c_int64(0)
        _check(self._h, lib.pisces_hip_flush_view(self._h, -1 if upToPosition is None else int(upToPosition), C.byref(rows), C.byref(n), None, None, None, None, None))
        return self._rows_at(rows, n.value)

    def CallEndView(self):
        """pisces_hip_flush_end_view: CallEnd() without the copy (valid until the next Call* / CallBegin)."""
        rows, n = C.c_void_p(), C.c_int64(0)
        _check(self._h, lib.pisces_hip_flush_end_view(self._h, C.byref(rows), C.byref(n), None, None, None, None, None))
        return self._rows_at(rows, n.value)

    @staticmethod
    def _rows_at(rows, n):
        if not n:
            return np.zeros(0, dtype=_abi.CALLED_ALLELE_DTYPE)
        # (through the array interface: a ctypes array type per row count is ~5 us of Python a flush, this is ~2)
        w = _RowsAt()
        w.__array_interface__ = {"shape": (n,), "typestr": "|V%d" % _abi.CALLED_ALLELE_DTYPE.itemsize, "data": (rows.value, False), "version": 3}
        return np.asarray(w).view(_abi.CALLED_ALLELE_DTYPE)

    def Posteriors(self, capacity=1 << 16):
        """CalledAllele.GenotypePosteriors of the rows the last Call* returned (pisces_hip_get_posteriors): a POSTERIORS_DTYPE array, row i
        of it for row i of the rows; n = 0 where a row has none (every row of a handle that is not PLOIDY_DIPLOID_ADAPTIVE)."""
        while True:
            out = np.zeros(capacity, dtype=_abi.POSTERIORS_DTYPE)
            n = C.c_int64(0)
            rc = lib.pisces_hip_get_posteriors(self._h, out.ctypes.data, len(out), C.byref(n))
            if rc == _abi.E_BUFFER_TOO_SMALL:
                capacity = int(n.value)
                continue
            _check(self._h, rc)
            return out[: n.value]

    def PosteriorsView(self):
        """pisces_hip_posteriors_view: Posteriors() without the copy, valid as long as the rows of CallView / CallEndView are."""
        rows, n = C.c_void_p(), C.c_int64(0)
        _check(self._h, lib.pisces_hip_posteriors_view(self._h, C.byref(rows), C.byref(n)))
        if not n.value:
            return np.zeros(0, dtype=_abi.POSTERIORS_DTYPE)
        w = _RowsAt()
        w.__array_interface__ = {"shape": (n.value,), "typestr": "|V%d" % _abi.POSTERIORS_DTYPE.itemsize, "data": (rows.value, False), "version": 3}
        return np.asarray(w).view(_abi.POSTERIORS_DTYPE)

    def SetAdaptiveGenotypingParameters(self, snv_model=None, indel_model=None, snv_prior=None, indel_prior=None, sum_vf_for_multi_allelic_site=None,
                                        max_genotype_posteriors=None):
        """AdaptiveGenotypingParameters of a PLOIDY_DIPLOID_ADAPTIVE caller (pisces_hip_set_adaptive_params); what is not given keeps the
        reference's default."""
        self._adaptive = adaptive_params(snv_model, indel_model, snv_prior, indel_prior, sum_vf_for_multi_allelic_site, max_genotype_posteriors)
        _check(self._h, lib.pisces_hip_set_adaptive_params(self._h, C.byref(self._adaptive)))

    def CallBegin(self, upToPosition=None):
        """pisces_hip_flush_begin: the flush enqueued, DoneProcessing committed; the alleles come with CallEnd.  In between the next
        reads may be staged and added."""
        _check(self._h, lib.pisces_hip_flush_begin(self._h, -1 if upToPosition is None else int(upToPosition)))

    def CallEnd(self, capacity=1 << 16, reuse_buffer=False):
        """pisces_hip_flush_end: the alleles of the flush CallBegin started (the rows Call would have returned)."""
        while True:
            if reuse_buffer:
                out = getattr(self, "_flush_out", None)
                if out is None or len(out) < capacity:
                    out = self._flush_out = np.zeros(capacity, dtype=_abi.CALLED_ALLELE_DTYPE)
            else:
                out = np.zeros(capacity, dtype=_abi.CALLED_ALLELE_DTYPE)
            n = C.c_int64(0)
            rc = lib.pisces_hip_flush_end(self._h, out.ctypes.data, len(out), C.byref(n))
            if rc == _abi.E_BUFFER_TOO_SMALL:
                capacity = int(n.value)
                continue
            _check(self._h, rc)
            return out[: n.value]

    def CallWithAlleles(self, upToPosition=None, capacity=1 << 16):
        """Call() that also returns the (ref, alt) allele strings of every row: Reference / SNV rows from the record's
        base codes, insertion / deletion rows from the candidate the library found (pisces_hip_flush_ex)."""
        up_to = -1 if upToPosition is None else int(upToPosition)
        return self._rows_with_alleles(lambda *outputs: lib.pisces_hip_flush_ex(self._h, up_to, *outputs), capacity)

    def CallEndWithAlleles(self, capacity=1 << 16):
        """CallEnd() with the allele strings (pisces_hip_flush_end_ex): what CallWithAlleles would have returned for the flush
        CallBegin started."""
        return self._rows_with_alleles(lambda *outputs: lib.pisces_hip_flush_end_ex(self._h, *outputs), capacity)

    def _rows_with_alleles(self, entry, capacity):
        cand_cap, pool_cap = 1024, 1 << 16
        while True:
            out = np.zeros(capacity, dtype=_abi.CALLED_ALLELE_DTYPE)
            idx = np.zeros(capacity, dtype=np.int32)
            cands = (_abi.PiscesCandidate * cand_cap)()
            pool = np.zeros(pool_cap, dtype=np.uint8)
            n, nc, nb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            rc = entry(out.ctypes.data, capacity, C.byref(n), idx.ctypes.data, cands, cand_cap, C.byref(nc), pool.ctypes.data, pool_cap, C.byref(nb))
            if rc == _abi.E_BUFFER_TOO_SMALL:
                capacity = max(capacity, int(n.value))
                cand_cap = max(cand_cap, int(nc.value))
                pool_cap = max(pool_cap, int(nb.value))
                continue
            _check(self._h, rc)
            recs = out[: n.value]
            # (point rows in one pass over the array; only the rows that stand on a candidate are looked up one by one)
            letters = np.array(list(_abi.BASE_OF_ALLELE) + ["?", "?"])
            info = recs["info"].astype(np.int64)
            alleles = list(zip(letters[_abi.info_ref(info)].tolist(), letters[_abi.info_alt(info)].tolist()))
            for i in np.nonzero(idx[: n.value] >= 0)[0].tolist():
                c = cands[idx[i]]
                o = c.allele_offset
                alleles[i] = (bytes(pool[o: o + c.ref_len]).decode("latin-1"), bytes(pool[o + c.ref_len: o + c.ref_len + c.alt_len]).decode("latin-1"))
            return recs, alleles

    def GetCandidates(self, upToPosition=None):
        """The insertion / deletion candidates held by the state manager: list of dicts."""
        up_to = -1 if upToPosition is None else int(upToPosition)
        n, nb = C.c_int64(0), C.c_int64(0)
        _check(self._h, lib.pisces_hip_get_candidates(self._h, up_to, None, 0, C.byref(n), None, 0, C.byref(nb)))
        cands = (_abi.PiscesCandidate * max(1, n.value))()
        pool = np.zeros(max(1, nb.value), dtype=np.uint8)
        _check(self._h, lib.pisces_hip_get_candidates(self._h, up_to, cands, n.value, C.byref(n), pool.ctypes.data, nb.value, C.byref(nb)))
        out = []
        for i in range(n.value):
            c = cands[i]
            o = c.allele_offset
            out.append({"position": c.position, "category": c.category, "ref": bytes(pool[o: o + c.ref_len]).decode("latin-1"),
                        "alt": bytes(pool[o + c.ref_len: o + c.ref_len + c.alt_len]).decode("latin-1"),
                        "support_by_dir": list(c.support_by_dir), "well_anchored_by_dir": list(c.well_anchored_by_dir),
                        "open_left": bool(c.open_left), "open_right": bool(c.open_right)})
        return out

    @staticmethod
    def _candidate_arrays(items):
        """[(position, ref, alt)] or [dict(position, category, ref, alt, support_by_dir, ...)] -> (PiscesCandidate[], allele pool)."""
        arr = (_abi.PiscesCandidate * max(1, len(items)))()
        pool = bytearray()
        for i, it in enumerate(items):
            d = it if isinstance(it, dict) else {"position": it[0], "ref": it[1], "alt": it[2]}
            c = arr[i]
            c.position, c.category = int(d["position"]), int(d.get("category", 0))
            c.ref_len, c.alt_len = len(d["ref"]), len(d["alt"])
            for k in range(3):
                c.support_by_dir[k] = int(d.get("support_by_dir", (0, 0, 0))[k])
                c.well_anchored_by_dir[k] = int(d.get("well_anchored_by_dir", (0, 0, 0))[k])
            c.open_left, c.open_right = int(bool(d.get("open_left", False))), int(bool(d.get("open_right", False)))
            c.allele_offset = len(pool)
            pool += d["ref"].encode() + d["alt"].encode()
        return arr, np.frombuffer(bytes(pool) or b"\0", dtype=np.uint8).copy(), len(pool)

    def AddCandidates(self, candidates):
        """IStateManager.AddCandidates for candidates the caller brings itself (dicts as GetCandidates returns them)."""
        arr, pool, nb = self._candidate_arrays(list(candidates))
        _check(self._h, lib.pisces_hip_add_candidates(self._h, arr, len(candidates), pool.ctypes.data, nb))

    def SetForcedAlleles(self, alleles):
        """-forcedalleles: [(position, ref, alt)] of this chromosome (AlleleCaller.AddForcedGtAlleles + SmallVariantCaller's forced
        candidates).  After SetIntervals, before the first Call."""
        arr, pool, nb = self._candidate_arrays(list(alleles))
        _check(self._h, lib.pisces_hip_set_forced_alleles(self._h, arr, len(alleles), pool.ctypes.data, nb))

    def SetExactTotalNumCalled(self, on=True):
        """pisces_hip_set_exact_total_called: TotalNumCalled also counts the callable SNVs outside the interval set (AlleleCaller.cs:109-131)."""
        _check(self._h, lib.pisces_hip_set_exact_total_called(self._h, int(bool(on))))

    def SetKnownVariants(self, variants):
        """The chromosome's known (prior) variants, [(position, ref, alt)]: Factory.cs:204 hands them to VariantCollapser (AnnotateKnown,
        VariantCollapser.cs:178-190).  [] clears."""
        arr, pool, nb = self._candidate_arrays(list(variants))
        _check(self._h, lib.pisces_hip_set_known_variants(self._h, arr, len(variants), pool.ctypes.data, nb))

    def SetExcludeMNVsFromCollapsing(self, on=True):
        """PiscesApplicationOptions.ExcludeMNVsFromCollapsing (VariantCollapser.cs:33): MNV candidates are no targets of the collapser."""
        _check(self._h, lib.pisces_hip_set_exclude_mnvs_from_collapsing(self._h, int(bool(on))))

    # ---- multi-GPU summary (one process per GPU): RCCL bound at run time by the library ----
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id made by rank 0 and handed to the other processes."""
        buf = (C.c_uint8 * 128)()
        rc = lib.pisces_hip_comm_unique_id(buf, 128)
        if rc != 0:
            raise PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode(errors="replace"))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(self._h, lib.pisces_hip_comm_init(self._h, buf, int(rank), int(world)))

    @staticmethod
    def comm_library():
        """pisces_hip_comm_library: '<source>: <path>' of the librccl the library binds (source = PISCES_HIP_RCCL_PATH | mapped | default)."""
        buf = C.create_string_buffer(4096)
        rc = lib.pisces_hip_comm_library(buf, len(buf))
        if rc < 0:
            raise PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode(errors="replace"))
        return buf.value.decode()

    def comm_ranks(self):
        """ncclCommCount of the handle's communicator (1 without one)."""
        n = C.c_int32(0)
        _check(self._h, lib.pisces_hip_comm_ranks(self._h, C.byref(n)))
        return int(n.value)

    def reduce_summary(self, values):
        """In-place sum over the ranks of the int64[4] summary (identity without a communicator)."""
        v = (C.c_int64 * 4)(*[int(x) for x in values])
        _check(self._h, lib.pisces_hip_reduce_summary(self._h, v))
        return [int(x) for x in v]

    def FindCandidates(self, reads, snvs_and_mnvs=True, call_mnvs=False, max_mnv_length=3, max_gap_between_mnv=1):
        """ICandidateVariantFinder.FindCandidates on the device (pisces_hip_find_candidates_device: the kernels pisces_hip_add_reads
        enqueues), against the reference given to SetReference: list of dicts per read event, unmerged, in read order."""
        batch = reads if isinstance(reads, _abi.ReadBatch) else _abi.ReadBatch(reads)
        cap, pool_cap = 4096, 1 << 18
        while True:
            cands = (_abi.PiscesCandidate * cap)()
            pool = np.zeros(pool_cap, dtype=np.uint8)
            nb = C.c_int64(0)
            n = lib.pisces_hip_find_candidates_device(self._h, C.byref(batch.c), int(snvs_and_mnvs), int(call_mnvs), max_mnv_length,
                                                      max_gap_between_mnv, cands, cap, pool.ctypes.data, pool_cap, C.byref(nb))
            if n == _abi.E_BUFFER_TOO_SMALL:
                cap *= 4
                pool_cap = max(pool_cap * 4, int(nb.value))
                continue
            if n < 0:
                _check(self._h, int(n))
            return _candidate_dicts(cands, pool, n)

    def Stats(self):
        s = (C.c_int64 * 4)()
        _check(self._h, lib.pisces_hip_stats(self._h, s))
        # SmallVariantCaller.cs:114-115 / AlignmentsSource.cs:63: the vector a multi-GPU job adds up over its interval shards
        return {"TotalNumCalled": s[0], "TotalNumCollapsed": s[1], "reads": s[2], "reads_skipped": s[3]}

    def HostTime(self, reset=False):
        """pisces_hip_host_time: where the host's time went inside the streaming surface."""
        t = (C.c_double * 4)()
        _check(self._h, lib.pisces_hip_host_time(self._h, t, 1 if reset else 0))
        flushes = int(t[3])
        return {"add_reads_s": t[0], "flush_s": t[1], "flush_wait_s": t[2], "flushes": flushes,
                "host_ms_per_flush": (t[1] - t[2]) / flushes * 1e3 if flushes else 0.0}

    def TransferBytes(self, reset=False):
        """pisces_hip_transfer_bytes: what crossed PCIe for this caller since the last reset."""
        b = (C.c_int64 * 4)()
        _check(self._h, lib.pisces_hip_transfer_bytes(self._h, b, 1 if reset else 0))
        return {"h2d_reads": int(b[0]), "d2h_records": int(b[1]), "d2h_candidates": int(b[2]), "d2h_counts": int(b[3])}

    # ---- device-resident surface ----
    def stream_handle(self):
        """pisces_hip_get_stream: the handle's own hipStream_t as an int (what stream=None stands for in the calls below)."""
        s = C.c_void_p()
        _check(self._h, lib.pisces_hip_get_stream(self._h, C.byref(s)))
        return int(s.value or 0)

    def torch_stream(self):
        """The handle's own stream as a torch.cuda.ExternalStream.  Tensors a torch host hands to the device-resident surface are
        allocated / filled under `with torch.cuda.stream(caller.torch_stream()):` so that torch's fill kernels and the library's launches
        sit in ONE queue: the handle's stream is hipStreamNonBlocking and does not order against torch's default (null) stream."""
        ts = getattr(self, "_torch_stream", None)
        if ts is None:
            import torch
            ts = self._torch_stream = torch.cuda.ExternalStream(self.stream_handle(), device=torch.device("cuda", self.device))
        return ts

    @staticmethod
    def _stream_arg(stream):
        """None = the handle's own stream (an explicit choice); a torch stream or a raw hipStream_t otherwise.  The null stream (0, e.g.
        torch.cuda.current_stream().cuda_stream of a default torch context) is refused: the C ABI reads NULL as "the handle's stream", which
        does not order against the null stream, so work torch queued there (a torch.zeros fill) would race the launch."""
        if stream is None:
            return None
        raw = int(getattr(stream, "cuda_stream", stream))
        if raw == 0:
            raise ValueError("stream 0 is HIP's null stream, which the handle's non-blocking stream is not ordered against: pass None (the handle's "
                             "own stream, after synchronizing your fills) or allocate under caller.torch_stream() and pass that")
        return raw

    def call_tiles(self, d_tuples, d_tiles, n_tiles, d_ref, ref_start, ref_len, d_records, capacity, d_tile_results, stream=None, posteriors=None):
        """All pointer arguments are raw device addresses (ints); capacity >= 256 * n_tiles record slots.  posteriors (a
        PLOIDY_DIPLOID_ADAPTIVE caller): a device tensor of 32 * capacity bytes, slot-parallel to the records, that this and every later
        launch fills (pisces_hip_set_posteriors_buffer)."""
        if posteriors is not None:
            _check(self._h, lib.pisces_hip_set_posteriors_buffer(self._h, posteriors.data_ptr(), posteriors.numel() * posteriors.element_size() // 32))
        _check(self._h, lib.pisces_hip_call_tiles(self._h, d_tuples, d_tiles, n_tiles, d_ref, ref_start, ref_len,
                                                  d_records, capacity, d_tile_results, self._stream_arg(stream)))

    def balanced_tile_loci(self, n_loci):
        """Tile size (<= 64) that gives every CU the same number of tiles for a launch over n_loci loci (pisces_hip_balanced_tile_loci)."""
        return int(lib.pisces_hip_balanced_tile_loci(self._h, int(n_loci)))

    def call_tiles_batched(self, batches, stream=None):
        """pisces_hip_call_tiles_batched: batches = list of (d_tuples, d_tiles, n_tiles, d_ref, ref_start, ref_len, d_records, capacity,
        d_tile_results) with per-batch output buffers; spread over the handle's lanes.  Waits for `stream` first when given; the outputs
        are complete after synchronize()."""
        arr = (_abi.PiscesTileBatch * max(len(batches), 1))()
        for i, (tu, ti, n, rf, rs, rl, rec, cap, tr) in enumerate(batches):
            arr[i].d_tuples, arr[i].d_tiles, arr[i].n_tiles, arr[i].ref_start_position = tu, ti, n, rs
            arr[i].d_ref_bases, arr[i].ref_length, arr[i].d_records, arr[i].d_tile_results, arr[i].record_capacity = rf, rl, rec, tr, cap
        _check(self._h, lib.pisces_hip_call_tiles_batched(self._h, arr, len(batches), self._stream_arg(stream)))

    def call_tiles_graph_build(self, batches):
        """pisces_hip_call_tiles_graph_build: the launches of `batches` (as call_tiles_batched takes them), in order, as one HIP graph."""
        arr = (_abi.PiscesTileBatch * max(len(batches), 1))()
        for i, (tu, ti, n, rf, rs, rl, rec, cap, tr) in enumerate(batches):
            arr[i].d_tuples, arr[i].d_tiles, arr[i].n_tiles, arr[i].ref_start_position = tu, ti, n, rs
            arr[i].d_ref_bases, arr[i].ref_length, arr[i].d_records, arr[i].d_tile_results, arr[i].record_capacity = rf, rl, rec, tr, cap
        gid = C.c_int32(-1)
        _check(self._h, lib.pisces_hip_call_tiles_graph_build(self._h, arr, len(batches), C.byref(gid)))
        return gid.value

    def call_tiles_graph_launch(self, graph_id, stream=None):
        _check(self._h, lib.pisces_hip_call_tiles_graph_launch(self._h, int(graph_id), self._stream_arg(stream)))

    def compact_records(self, d_records, d_tile_results, n_tiles, d_offsets, d_out, out_capacity, d_count, stream=None):
        _check(self._h, lib.pisces_hip_compact_records(self._h, d_records, d_tile_results, n_tiles, d_offsets, d_out,
                                                       out_capacity, d_count, self._stream_arg(stream)))

    def compact_posteriors(self, d_posteriors, d_tile_results, n_tiles, d_offsets, d_out, out_capacity, stream=None):
        """pisces_hip_compact_posteriors: after compact_records, with the d_offsets it filled."""
        _check(self._h, lib.pisces_hip_compact_posteriors(self._h, d_posteriors, d_tile_results, n_tiles, d_offsets, d_out, out_capacity,
                                                          self._stream_arg(stream)))

    def format_vcf_device(self, chrom, d_recs, n, vcf_config=None, d_count=None, d_cand_index=None, d_cands=None, d_alleles=None, d_gp=None,
                          capacity=None, line_offsets=False, stream=None, **overrides):
        """pisces_hip_format_vcf_device: the VCF body lines of `n` (or min(n, *d_count)) device-resident rows, written on the device and
        returned as bytes — what format_vcf returns for the same rows, encoded.  Every d_* is a torch tensor or a raw device address;
        d_count is the word compact_records leaves, d_cand_index / d_cands / d_alleles what CallWithAlleles' candidates are in device
        memory, d_gp the compacted posteriors (the :GP column).  vcf_config / overrides as format_vcf takes them (indel_repeat_filter included; crush is refused).
        The launches go to `stream` (None = the handle's own) behind whatever made the rows; the call then waits once, for the size
        word, and repeats with a buffer of that size when `capacity` (default 128 bytes a row) was short.  line_offsets=True returns
        (text, offsets) with the rows + 1 byte offsets of the lines as a numpy int64 array."""
        import torch
        cfg = vcf_config
        if cfg is None:
            cfg = _abi.PiscesVcfConfig()
            _check(None, lib.pisces_hip_vcf_default_config(C.byref(cfg)))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        ptr = lambda t: None if t is None else (int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t))
        raw = self._stream_arg(stream)
        ts = self.torch_stream() if raw is None else torch.cuda.ExternalStream(raw, device=torch.device("cuda", self.device))
        dev = torch.device("cuda", self.device)
        n = int(n)
        cap = int(capacity) if capacity is not None else 128 * max(n, 1)
        size_word = torch.zeros(1, dtype=torch.int64).pin_memory()   # the kernel's own store into pinned memory: one stream wait, no copy
        with torch.cuda.stream(ts):
            offs = torch.full((n + 1,), -1, dtype=torch.int64, device=dev) if line_offsets else None
            for _ in range(2):
                text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
                _check(self._h, lib.pisces_hip_format_vcf_device(self._h, C.byref(cfg), chrom.encode(), ptr(d_recs), n, ptr(d_count), ptr(d_cand_index),
                                                                 ptr(d_cands), ptr(d_alleles), ptr(d_gp), text.data_ptr(), cap, ptr(offs),
                                                                 size_word.data_ptr(), ts.cuda_stream))
                ts.synchronize()
                need = int(size_word[0])
                if need < 0:
                    raise PiscesHipError(need, "format_vcf_device: a row the host formatter refuses too (a filter bit whose name the configuration "
                                               "does not give, or a candidate index without candidates)")
                if need <= cap:
                    break
                cap = need
            out = bytes(text[:need].cpu().numpy().tobytes())
            if line_offsets:
                written = offs.cpu().numpy()
                return out, written[written >= 0]   # the rows + 1 entries the kernels wrote: min(n, *d_count) lines, then the total
            return out

    def vqr_count_device(self, d_recs, n, d_counts, options=None, d_count=None, lo=0, hi=None, d_suspect=None, stream=None):
        """pisces_hip_vqr_count_device: VariantQualityRecalibration's counting pass over rows [lo, hi) of the device-resident rows
        d_recs[0, min(n, *d_count)), ADDED into d_counts (a device int64 tensor of 2 * 17 words, PiscesVqrCounts[2]: zero it once, the
        calls of several chromosomes sum).  With options.do_amplicon_position_checks d_suspect (n bytes) receives the suspect byte of
        every counted row.  Every d_* is a torch tensor or a raw device address.  Asynchronous on `stream` (None = the handle's own)."""
        opts = options if options is not None else vqr_options()
        ptr = lambda t: None if t is None else (int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t))
        n = int(n)
        _check(self._h, lib.pisces_hip_vqr_count_device(self._h, C.byref(opts), ptr(d_recs), n, ptr(d_count), int(lo), n if hi is None else int(hi),
                                                        ptr(d_counts), ptr(d_suspect), self._stream_arg(stream)))

    def vqr_apply_device(self, d_recs, n, tables, options=None, d_count=None, d_suspect=None, d_n_changed=None, stream=None):
        """pisces_hip_vqr_apply_device: the update pass over d_recs[0, min(n, *d_count)), in place, with the tables of vqr_tables and the
        suspect bytes the counting pass left for the same rows; *d_n_changed (a device int64, optional) is ADDED the rows rewritten.
        Asynchronous on `stream`."""
        opts = options if options is not None else vqr_options()
        ptr = lambda t: None if t is None else (int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t))
        _check(self._h, lib.pisces_hip_vqr_apply_device(self._h, C.byref(opts), C.byref(tables), ptr(d_recs), int(n), ptr(d_count), ptr(d_suspect),
                                                        ptr(d_n_changed), self._stream_arg(stream)))

    def venn_consensus_device(self, rows_a, rows_b, out, options=None, stream=None):
        """pisces_hip_venn_consensus_device: VennVcf's consensus of two probe pools' device-resident rows of one chromosome (rows_a, rows_b:
        venn_rows(...) over torch tensors or raw device addresses; out: venn_out(...), whose n_out is a device-accessible int64[3] that
        receives rows, candidates and allele bytes — or {PISCES_E_INVALID_ARG, pool, row} for an unsorted pool; nothing else is written when
        a count is above its capacity).  Asynchronous on `stream` (None = the handle's own)."""
        opts = options if options is not None else venn_options()
        _check(self._h, lib.pisces_hip_venn_consensus_device(self._h, C.byref(opts), C.byref(rows_a), C.byref(rows_b), C.byref(out), self._stream_arg(stream)))

    def vead_groups_device(self, sites, neighborhoods, out, batch=None, options=None, stream=None):
        """pisces_hip_vead_groups_device: Scylla's read pass over reads in device memory.  sites: vead_sites([(position, ref, alt), ...]);
        neighborhoods: [(site_begin, site_end), ...] into them; batch: a DeviceReadBatch, or None for the batch bam_decode left on the
        device; out: vead_out(...) over torch tensors or raw device addresses, whose n_out is a device-accessible int64[3] that receives
        groups, state bytes and 0 (only n_out and info are written when a count is above its capacity).  The call waits once for the
        neighbourhoods' read ranges, everything behind that is asynchronous on `stream` (None = the handle's own)."""
        opts = options if options is not None else vead_options()
        site_rows, alleles = sites
        nb = _vead_neighborhoods(neighborhoods)
        _check(self._h, lib.pisces_hip_vead_groups_device(self._h, C.byref(opts), C.byref(batch.c) if batch is not None else None,
                                                          batch.n_ops if batch is not None else 0, batch.n_bases if batch is not None else 0,
                                                          site_rows.ctypes.data, len(site_rows), alleles.ctypes.data, alleles.size, nb.ctypes.data, len(nb),
                                                          C.byref(out), self._stream_arg(stream)))

    def nbhd_build_device(self, rows, out, criteria=None, stream=None):
        """pisces_hip_nbhd_build_device: Scylla's neighbourhoods from the device-resident rows of one chromosome (rows: venn_rows(...); out:
        nbhd_out(...) over torch tensors, pinned host arrays or raw addresses, whose n_out is a device-accessible int64[6] that receives
        kept neighbourhoods, sites, allele bytes, reference bytes, raw neighbourhoods and eligible rows — or an error word; nothing else
        is written when a count is above its capacity).  Asynchronous on `stream` (None = the handle's own), no host wait inside."""
        crit = criteria if criteria is not None else nbhd_criteria()
        _check(self._h, lib.pisces_hip_nbhd_build_device(self._h, C.byref(crit), C.byref(rows), C.byref(out), self._stream_arg(stream)))

    def phase_evidence_device(self, rows, batch=None, criteria=None, options=None, stream=None):
        """What a Scylla host does with rows and reads that lie on the device: the neighbourhood tables of `rows` (venn_rows(...)) built
        into pinned host arrays (counts first, then the sizes they ask for), one wait, then the tables handed to vead_groups_device over
        `batch` (None: the batch bam_decode left on the device).  Returns {"nbhd": the tables as nbhd_build gives them, "groups", "states",
        "info"}: the read pass's arrays.  An error word of the build raises PiscesHipError; the read pass's refusals (a neighbourhood above
        VEAD_MAX_SITES among them) pass through unchanged."""
        import torch
        dev = torch.device("cuda", self.device)
        wait = (lambda: self.synchronize()) if stream is None else (lambda: torch.cuda.synchronize(dev))
        pinned = lambda nbytes: torch.zeros(max(int(nbytes), 1), dtype=torch.uint8).pin_memory()
        n = int(rows.n)
        n_out = pinned(48)
        caps = (0, 0, 0, 0)
        while True:
            t = {"sites": pinned(caps[1] * 16), "alleles": pinned(caps[2]), "site_row": pinned(caps[1] * 4), "site_original": pinned(caps[1] * 4),
                 "neighbourhoods": pinned(caps[0] * 8), "info": pinned(caps[0] * 48), "ref_bytes": pinned(caps[3]), "row_class": pinned(n)}
            out = nbhd_out(t["sites"], t["alleles"], t["site_row"], t["site_original"], t["neighbourhoods"], t["info"], t["ref_bytes"], n_out, *caps,
                           row_class=t["row_class"])
            self.nbhd_build_device(rows, out, criteria, stream)
            wait()
            counts = [int(v) for v in n_out.numpy()[:48].view(np.int64)]
            if counts[0] < 0:
                raise _nbhd_error_word(counts)
            if all(c <= cap for c, cap in zip(counts[:4], caps)):
                break
            caps = tuple(counts[:4])
        nbhd = _nbhd_result({k: v.numpy() for k, v in t.items()}, counts, n)
        sites = (nbhd["sites"], nbhd["alleles"])
        vead_n_out = pinned(24)
        vcaps = (0, 0)
        while True:
            with torch.cuda.stream(self.torch_stream()):
                groups = torch.zeros(max(vcaps[0], 1) * 24, dtype=torch.uint8, device=dev)
                states = torch.zeros(max(vcaps[1], 1), dtype=torch.uint8, device=dev)
                info = torch.zeros(max(counts[0], 1) * 32, dtype=torch.uint8, device=dev)
            self.synchronize()
            self.vead_groups_device(sites, nbhd["neighbourhoods"], vead_out(groups, states, info, vead_n_out, *vcaps), batch=batch, options=options, stream=stream)
            wait()
            got = [int(v) for v in vead_n_out.numpy()[:24].view(np.int64)]
            if got[0] <= vcaps[0] and got[1] <= vcaps[1]:
                break
            vcaps = (got[0], got[1])
        return {"nbhd": nbhd, "groups": groups.cpu().numpy()[:got[0] * 24].view(_abi.VEAD_GROUP_DTYPE).copy(), "states": states.cpu().numpy()[:got[1]].copy(),
                "info": info.cpu().numpy()[:counts[0] * 32].view(_abi.VEAD_INFO_DTYPE).copy()}

    def accumulate_tiles(self, d_tuples, d_tiles, n_tiles, d_counts, stream=None):
        _check(self._h, lib.pisces_hip_accumulate_tiles(self._h, d_tuples, d_tiles, n_tiles, d_counts, self._stream_arg(stream)))

    def device_totals(self, reset=False):
        """{records, candidate_loci, called (IAlleleCaller.TotalNumCalled), tiles} summed over call_tiles launches."""
        s = (C.c_int64 * 4)()
        _check(self._h, lib.pisces_hip_device_totals(self._h, s, 1 if reset else 0))
        return {"records": s[0], "candidate_loci": s[1], "called": s[2], "tiles": s[3]}

    def mark(self, which, stream=None):
        """pisces_hip_mark: an event on the launch stream in front of (0) / behind (1) a run of launches."""
        _check(self._h, lib.pisces_hip_mark(self._h, int(which), self._stream_arg(stream)))

    def marked_ms(self):
        ms = C.c_float(0)
        _check(self._h, lib.pisces_hip_marked_ms(self._h, C.byref(ms)))
        return ms.value

    def set_timing(self, enable=True):
        """enable = True / n > 0: time every launch / every n-th launch with HIP events; False / 0: off (default)."""
        _check(self._h, lib.pisces_hip_set_timing(self._h, int(enable)))

    def kernel_time(self):
        """(total_ms, launches) of the kernels launched since set_timing(True), from HIP events on the launch stream."""
        ms, n = C.c_double(0), C.c_int64(0)
        _check(self._h, lib.pisces_hip_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def SetChainTiming(self, enable=True):
        """pisces_hip_set_chain_timing: events around what AddDeviceReads enqueues and around a flush's kernels (up to the compacted records)."""
        _check(self._h, lib.pisces_hip_set_chain_timing(self._h, int(bool(enable))))

    def ChainTime(self):
        """(add_ms, flush_ms) of the last AddDeviceReads and the last flush since SetChainTiming(True): device time by HIP events."""
        out = (C.c_double * 2)()
        _check(self._h, lib.pisces_hip_chain_time(self._h, out))
        return out[0], out[1]

    def probe_read_bandwidth(self, nbytes=1 << 30, reps=6):
        """GB/s of a plain streaming read on this device (context for the roofline fraction)."""
        g = C.c_double(0)
        _check(self._h, lib.pisces_hip_probe_read_bandwidth(self._h, nbytes, reps, C.byref(g)))
        return g.value

    def synchronize(self):
        _check(self._h, lib.pisces_hip_synchronize(self._h))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        _check(self._h, lib.pisces_hip_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def bgzf_inflate(self, file_bytes, check_crc=True):
        """Row f4 (upstream): every BGZF block of `file_bytes` (a BAM file or a region of one) inflated on the device, one wave per
        block (BamReader.ReadBlock -> UncompressBlock, BamReader.cs:603-645).  Returns (inflated bytes, block table, kernel ms)."""
        data = np.frombuffer(bytes(file_bytes), dtype=np.uint8)
        blocks, total = bgzf_scan(data)
        out = np.zeros(max(total, 1), dtype=np.uint8)
        ms = C.c_float(0)
        _check(self._h, lib.pisces_hip_bgzf_inflate(self._h, data.ctypes.data, data.size, blocks, len(blocks), out.ctypes.data, total,
                                                    1 if check_crc else 0, C.byref(ms)))
        return out[:total].tobytes(), blocks, ms.value

    def bam_decode(self, file_bytes, ref_id, min_map_quality=1, skip_duplicates=True, only_proper_pairs=False):
        """Row f4: a BAM file (bytes, or the array bam_stage returned) inflated and cut into records on the device; the alignments of
        reference sequence `ref_id` that AlignmentSource.ShouldSkipRead keeps become a device-resident read batch.  Returns {reads,
        skipped, cigar_ops, bases}."""
        data = file_bytes if isinstance(file_bytes, np.ndarray) else np.frombuffer(bytes(file_bytes), dtype=np.uint8)
        blocks, _ = bgzf_scan(data)
        counts = (C.c_int64 * 4)()
        _check(self._h, lib.pisces_hip_bam_decode(self._h, data.ctypes.data, data.size, blocks, len(blocks), int(ref_id), int(min_map_quality),
                                                  int(bool(skip_duplicates)), int(bool(only_proper_pairs)), counts))
        self._bam_counts = {"reads": counts[0], "skipped": counts[1], "cigar_ops": counts[2], "bases": counts[3]}
        mode = lib.pisces_hip_bam_chain_mode(self._h)
        return dict(self._bam_counts, chain="guessed" if mode == 0 else "hopped")

    def bam_fetch_directions(self):
        """(directions, deletion_directions) of the decoded batch — made when some read of it carries the Stitcher's XD tag — or None."""
        n = self._bam_counts
        dirs, dd = np.zeros(n["bases"], np.uint8), np.zeros(2 * n["cigar_ops"], np.uint8)
        rc = lib.pisces_hip_bam_fetch_directions(self._h, dirs.ctypes.data, dd.ctypes.data)
        if rc < 0:
            _check(self._h, rc)
        return (dirs, dd) if rc == 1 else None

    def bam_fetch_amplicons(self):
        """The amplicon id of every read of the decoded batch (its XN tag as an id of AmpliconNames(), -1 without the tag), or None when
        the batch has none: the handle did not track amplicon counts when it was decoded."""
        ids = np.zeros(self._bam_counts["reads"], np.int32)
        rc = lib.pisces_hip_bam_fetch_amplicons(self._h, ids.ctypes.data)
        if rc < 0:
            _check(self._h, rc)
        return ids if rc == 1 else None

    def AmpliconNames(self):
        """The handle's amplicon names (bytes), index = id: what the decodes met, in order of first appearance, and InternAmpliconName's."""
        n = lib.pisces_hip_amplicon_name_count(self._h)
        if n < 0:
            _check(self._h, n)
        names = []
        for i in range(n):
            length = lib.pisces_hip_get_amplicon_name(self._h, i, None, 0)
            if length < 0:
                _check(self._h, length)
            buf = C.create_string_buffer(max(length, 1))
            _check(self._h, min(lib.pisces_hip_get_amplicon_name(self._h, i, buf, length), 0))
            names.append(buf.raw[:length])
        return names

    def InternAmpliconName(self, name):
        """The id of `name` (bytes or str) in the handle's dictionary, a new one when the name is new: for reads the host parses itself and
        hands to AddAlleleCounts(reads, amplicon_ids=...) beside decoded batches."""
        raw = name.encode() if isinstance(name, str) else bytes(name)
        rc = lib.pisces_hip_intern_amplicon_name(self._h, raw, len(raw))
        if rc < 0:
            _check(self._h, rc)
        return rc

    def bam_fetch(self):
        """The decoded batch as host arrays (dict with the PiscesReadBatch field names)."""
        n = self._bam_counts
        out = {"position": np.zeros(n["reads"], np.int32), "flags": np.zeros(n["reads"], np.uint8),
               "cigar_offset": np.zeros(n["reads"] + 1, np.int32), "cigar_op": np.zeros(n["cigar_ops"], np.uint8),
               "cigar_len": np.zeros(n["cigar_ops"], np.uint32), "seq_offset": np.zeros(n["reads"] + 1, np.int32),
               "bases": np.zeros(n["bases"], np.uint8), "quals": np.zeros(n["bases"], np.uint8)}
        _check(self._h, lib.pisces_hip_bam_fetch(self._h, *[out[k].ctypes.data for k in ("position", "flags", "cigar_offset", "cigar_op",
                                                                                       "cigar_len", "seq_offset", "bases", "quals")]))
        return out

    def AddDecodedReads(self):
        """AddAlleleCounts + FindCandidates for the batch bam_decode left on the device (bases and qualities never come back)."""
        _check(self._h, lib.pisces_hip_add_decoded_reads(self._h))


def device_count():
    """pisces_hip_device_count: the HIP devices of this process (a -threadbychr host gives job j the device j % count)."""
    n = lib.pisces_hip_device_count()
    if n < 0:
        raise PiscesHipError(n, "pisces_hip_device_count: no HIP runtime / device")
    return int(n)


def anchor_adjusted_count(c, minAnchor=0, maxAnchor=None, fromEnd=False, symmetric=False):
    """AlleleCountHelper.GetAnchorAdjustedAlleleCount (AlleleCountHelper.cs:21-85) over one [11] anchor row."""
    well = _abi.ANCHOR_SIZE
    n = _abi.NUM_ANCHORS
    true_min = min(well, minAnchor)
    init_max = well
    if maxAnchor is not None:
        init_max = well - 1 if maxAnchor >= well else maxAnchor
    tot = 0
    if fromEnd:
        for i in range(true_min, init_max + 1):
            tot += int(c[n - i - 1])
        if maxAnchor is None:
            for i in range(true_min if symmetric else 0, init_max):
                tot += int(c[i])
    else:
        for i in range(true_min, init_max + 1):
            tot += int(c[i])
        if maxAnchor is None:
            for i in range(init_max + 1, (n - true_min) if symmetric else n):
                tot += int(c[i])
    return tot


def expand_reads(batch, min_base_call_quality=20):
    """Host expansion of reads into (position, tuple) observations (pisces_hip_expand_reads)."""
    cap = batch.n_bases * 2 + 64
    while True:
        pos = np.zeros(cap, dtype=np.int32)
        tup = np.zeros(cap, dtype=np.uint32)
        n = lib.pisces_hip_expand_reads(C.byref(batch.c), min_base_call_quality, pos.ctypes.data, tup.ctypes.data, cap)
        if n == _abi.E_BUFFER_TOO_SMALL:
            cap *= 4
            continue
        if n < 0:
            raise PiscesHipError(int(n), "expand_reads failed")
        return pos[:n], tup[:n]


def adaptive_params(snv_model=None, indel_model=None, snv_prior=None, indel_prior=None, sum_vf_for_multi_allelic_site=None, max_genotype_posteriors=None):
    """_abi.PiscesAdaptiveParams: the reference's defaults (pisces_hip_adaptive_default_params) with the given members replaced"""
    p = _abi.PiscesAdaptiveParams()
    _check(None, lib.pisces_hip_adaptive_default_params(C.byref(p)))
    for name, v in (("snv_model", snv_model), ("indel_model", indel_model), ("snv_prior", snv_prior), ("indel_prior", indel_prior)):
        if v is not None:
            setattr(p, name, (C.c_double * 3)(*[float(x) for x in v]))
    if sum_vf_for_multi_allelic_site is not None:
        p.sum_vf_for_multi_allelic_site = float(sum_vf_for_multi_allelic_site)
    if max_genotype_posteriors is not None:
        p.max_genotype_posteriors = int(max_genotype_posteriors)
    return p


def set_genotypes_adaptive(alleles, config=None, params=None):
    """pisces_hip_set_genotypes_adaptive over the alleles of one locus: alleles = list of dicts(category, ref, alt, support, coverage[,
    reference_support]).  Returns (locus genotype, list of dicts(genotype, genotype_qscore, phase_set_index, multi_allelic, prune), posteriors
    as a POSTERIORS_DTYPE array)."""
    cfg = config if config is not None else _abi.default_config()
    par = params if params is not None else adaptive_params()
    n = len(alleles)
    arr = (_abi.PiscesGenotypeAllele * max(n, 1))()
    pool = bytearray()
    for i, a in enumerate(alleles):
        arr[i].category, arr[i].ref_len, arr[i].alt_len = int(a["category"]), len(a["ref"]), len(a["alt"])
        arr[i].support, arr[i].coverage, arr[i].reference_support = int(a["support"]), int(a["coverage"]), int(a.get("reference_support", 0))
        arr[i].allele_offset = len(pool)
        pool += a["ref"].encode() + a["alt"].encode()
    pool_arr = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy()
    post = np.zeros(max(n, 1), dtype=_abi.POSTERIORS_DTYPE)
    gt = lib.pisces_hip_set_genotypes_adaptive(C.byref(cfg), C.byref(par), arr, n, pool_arr.ctypes.data, len(pool), post.ctypes.data)
    if gt < 0:
        raise PiscesHipError(int(gt), "set_genotypes_adaptive failed")
    res = [dict(genotype=arr[i].genotype, genotype_qscore=arr[i].genotype_qscore, phase_set_index=arr[i].phase_set_index,
                multi_allelic=bool(arr[i].multi_allelic), prune=bool(arr[i].prune)) for i in range(n)]
    return int(gt), res, post[:n]


def adaptive_genotype_qscore(allele_support, total_coverage, category=_abi.CAT_SNV, is_reference=False, params=None):
    """pisces_hip_adaptive_genotype_qscore: (mixture component 0 / 1 / 2, q-score 0..100, three phred-scaled posteriors)"""
    par = params if params is not None else adaptive_params()
    cat, q = C.c_int32(0), C.c_int32(0)
    gp = (C.c_float * 3)()
    _check(None, lib.pisces_hip_adaptive_genotype_qscore(C.byref(par), int(category), int(bool(is_reference)), int(allele_support), int(total_coverage),
                                                         C.byref(cat), C.byref(q), gp))
    return cat.value, q.value, np.array(list(gp), dtype=np.float32)


def amplicon_bias(support, coverage, threshold):
    """pisces_hip_amplicon_bias for the amplicons of one SNV: (True / False / None for "no result", the chance of every amplicon or None)"""
    sup = np.ascontiguousarray(support, dtype=np.int32)
    cov = np.ascontiguousarray(coverage, dtype=np.int32)
    if sup.shape != cov.shape or sup.ndim != 1:
        raise PiscesHipError(_abi.E_INVALID_ARG, "amplicon_bias: support and coverage are two lists of one length")
    chance = np.zeros(len(sup), dtype=np.float64)
    i32p = C.POINTER(C.c_int32)
    rc = lib.pisces_hip_amplicon_bias(sup.ctypes.data_as(i32p), cov.ctypes.data_as(i32p), len(sup), float(threshold),
                                      chance.ctypes.data_as(C.POINTER(C.c_double)))
    return (None, None) if rc < 0 else (bool(rc), chance)


def indel_repeat_length(category, position, ref_allele, alt_allele, reference):
    """pisces_hip_indel_repeat_length: AlleleProcessor.ComputeIndelRepeatLength for one allele (category an _abi.CAT_* value, the alleles
    with their anchor base, reference[i] = position i + 1).  Raises PiscesHipError(E_INVALID_ARG) where the reference's Substring throws
    (a position decidedly outside the chromosome)."""
    as_bytes = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    r, a = as_bytes(ref_allele), as_bytes(alt_allele)
    ref = np.frombuffer(as_bytes(reference), dtype=np.uint8) if not isinstance(reference, np.ndarray) else np.ascontiguousarray(reference, np.uint8)
    rc = lib.pisces_hip_indel_repeat_length(int(category), int(position), r, len(r), a, len(a), ref.ctypes.data if ref.size else None, ref.size)
    if rc < 0:
        raise PiscesHipError(int(rc), f"indel_repeat_length: position {int(position)} is outside what a chromosome of {ref.size} bases can answer for "
                                      "(the reference throws ArgumentOutOfRangeException), or an allele lacks its anchor base")
    return rc


def vqr_options(**overrides):
    """PiscesVqrOptions with VQROptions' defaults (pisces_hip_vqr_default_options), fields overridden by name."""
    opts = _abi.PiscesVqrOptions()
    _check(None, lib.pisces_hip_vqr_default_options(C.byref(opts)))
    for k, v in overrides.items():
        if not hasattr(opts, k):
            raise AttributeError(f"PiscesVqrOptions has no field {k!r}")
        setattr(opts, k, v)
    return opts


def vqr_counts_array(counts=None):
    """PiscesVqrCounts[2] ([0] all rows, [1] rows at an edge), zeroed or filled from two (by_category[16], num_possible_variants) pairs."""
    arr = (_abi.PiscesVqrCounts * 2)()
    for k, (by_category, num_possible) in enumerate(counts or ()):
        arr[k].by_category[:] = [int(x) for x in by_category]
        arr[k].num_possible_variants = int(num_possible)
    return arr


def vqr_count(records, options=None, lo=0, hi=None, counts=None):
    """pisces_hip_vqr_count: the counting pass over host rows (a CALLED_ALLELE_DTYPE array).  Returns (counts, suspect): the
    PiscesVqrCounts[2] the rows [lo, hi) were added to (`counts`, or a zeroed pair) and the suspect bytes (None with the edge checks off)."""
    opts = options if options is not None else vqr_options()
    recs = np.ascontiguousarray(records, dtype=_abi.CALLED_ALLELE_DTYPE)
    n = len(recs)
    arr = counts if counts is not None else vqr_counts_array()
    suspect = np.zeros(max(n, 1), dtype=np.uint8) if opts.do_amplicon_position_checks else None
    _check(None, lib.pisces_hip_vqr_count(C.byref(opts), recs.ctypes.data if n else None, n, int(lo), n if hi is None else int(hi), arr,
                                          None if suspect is None else suspect.ctypes.data))
    return arr, (None if suspect is None else suspect[:n])


def vqr_tables(counts, options=None):
    """pisces_hip_vqr_tables: the recalibration tables (PiscesVqrTables) from a PiscesVqrCounts[2]; host only."""
    opts = options if options is not None else vqr_options()
    tables = _abi.PiscesVqrTables()
    _check(None, lib.pisces_hip_vqr_tables(C.byref(opts), counts, C.byref(tables)))
    return tables


def venn_options(**overrides):
    """PiscesVennOptions with VennVcf's defaults (pisces_hip_venn_default_options), fields overridden by name."""
    opts = _abi.PiscesVennOptions()
    _check(None, lib.pisces_hip_venn_default_options(C.byref(opts)))
    for k, v in overrides.items():
        if not hasattr(opts, k):
            raise AttributeError(f"PiscesVennOptions has no field {k!r}")
        setattr(opts, k, v)
    return opts


def _address(t):
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return int(t.data_ptr())
    if hasattr(t, "ctypes"):
        return int(t.ctypes.data)
    if isinstance(t, C.Array):
        return C.addressof(t)
    return int(t)


def venn_rows(recs, n, count=None, cand_index=None, cands=None, alleles=None):
    """PiscesVennRows: one pool's rows as a flush gives them out.  Every argument is a torch tensor, a numpy array, a ctypes array or a raw
    address; the caller keeps them alive."""
    r = _abi.PiscesVennRows()
    r.recs, r.n, r.count, r.cand_index, r.cands, r.alleles = _address(recs), int(n), _address(count), _address(cand_index), _address(cands), _address(alleles)
    return r


def venn_out(recs, cand_index, cands, alleles, n_out, row_capacity, cand_capacity, allele_capacity, info=None, venn_a=None, venn_b=None):
    """PiscesVennOut: where the consensus goes (see venn_rows for the argument kinds)."""
    o = _abi.PiscesVennOut()
    o.recs, o.cand_index, o.cands, o.alleles, o.info = _address(recs), _address(cand_index), _address(cands), _address(alleles), _address(info)
    o.venn_a, o.venn_b, o.n_out = _address(venn_a), _address(venn_b), _address(n_out)
    o.row_capacity, o.cand_capacity, o.allele_capacity = int(row_capacity), int(cand_capacity), int(allele_capacity)
    return o


_BASE_OF_CODE = "AGCTN"


def candidate_table(records, alleles):
    """(cand_index int32[n], PiscesCandidate[], allele bytes uint8[]) from the (ref, alt) string pairs of format_vcf: a pair of single
    bases (a Reference row's alt is ".") has no candidate and reads its alleles from the base codes of info."""
    idx_l, cand_l, pool = [], [], bytearray()
    for rec, (r, a) in zip(records, alleles):
        if len(r) == 1 and len(a) == 1:
            idx_l.append(-1)
            continue
        c = _abi.PiscesCandidate()
        c.position, c.category = int(rec["position"]), (int(rec["info"]) >> 4) & 7
        c.ref_len, c.alt_len, c.allele_offset = len(r), len(a), len(pool)
        pool += r.encode() + a.encode()
        idx_l.append(len(cand_l))
        cand_l.append(c)
    return (np.array(idx_l, dtype=np.int32), (_abi.PiscesCandidate * max(len(cand_l), 1))(*cand_l),
            np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy())


def venn_consensus(records_a, records_b, options=None, alleles_a=None, alleles_b=None, capacities=None):
    """pisces_hip_venn_consensus: VennVcf's consensus of two probe pools over host rows (CALLED_ALLELE_DTYPE arrays of one chromosome, sorted
    by position); alleles_a / alleles_b are format_vcf's (ref, alt) pairs for pools with insertion / deletion / MNV rows.  Returns a dict:
    records, cand_index, cands (PiscesCandidate[]), allele_bytes, alleles (the (ref, alt) pairs of the consensus rows), info
    (CONSENSUS_INFO_DTYPE), venn_a, venn_b (one class byte per input row), n_out (rows, candidates, allele bytes).  capacities: (rows,
    candidates, allele bytes) to offer instead of sizes that always fit; too small raises PiscesHipError(PISCES_E_BUFFER_TOO_SMALL) whose
    n_out attribute holds the three counts."""
    opts = options if options is not None else venn_options()
    pools, keep = [], []
    for recs, alleles in ((records_a, alleles_a), (records_b, alleles_b)):
        recs = np.ascontiguousarray(recs, dtype=_abi.CALLED_ALLELE_DTYPE)
        table = candidate_table(recs, alleles) if alleles is not None else (None, None, None)
        keep.append((recs, table))
        pools.append(venn_rows(recs if len(recs) else None, len(recs), None, *table))
    (ra, ta), (rb, tb) = keep
    n_in = len(ra) + len(rb)
    bytes_in = sum(len(t[2]) for t in (ta, tb) if t[2] is not None)
    caps = capacities if capacities is not None else (n_in, n_in, bytes_in)
    recs = np.zeros(max(caps[0], 1), dtype=_abi.CALLED_ALLELE_DTYPE)
    cand_index = np.full(max(caps[0], 1), -1, dtype=np.int32)
    cands = (_abi.PiscesCandidate * max(caps[1], 1))()
    pool = np.zeros(max(caps[2], 1), dtype=np.uint8)
    info = np.zeros(max(caps[0], 1), dtype=_abi.CONSENSUS_INFO_DTYPE)
    venn_a, venn_b = np.zeros(max(len(ra), 1), dtype=np.uint8), np.zeros(max(len(rb), 1), dtype=np.uint8)
    n_out = np.zeros(3, dtype=np.int64)
    out = venn_out(recs, cand_index, cands, pool, n_out, caps[0], caps[1], caps[2], info=info, venn_a=venn_a, venn_b=venn_b)
    rc = lib.pisces_hip_venn_consensus(C.byref(opts), C.byref(pools[0]), C.byref(pools[1]), C.byref(out))
    if rc != 0:
        err = PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode())
        err.n_out = [int(x) for x in n_out]
        raise err
    n, nc, nb = (int(x) for x in n_out)
    pairs = []
    for i in range(n):
        if cand_index[i] >= 0:
            c = cands[cand_index[i]]
            o = c.allele_offset
            pairs.append((bytes(pool[o: o + c.ref_len]).decode("latin-1"), bytes(pool[o + c.ref_len: o + c.ref_len + c.alt_len]).decode("latin-1")))
        else:
            word = int(recs["info"][i])
            is_ref = ((word >> 4) & 7) == _abi.CAT_REFERENCE
            pairs.append((_BASE_OF_CODE[min((word >> 7) & 7, 4)], "." if is_ref else _BASE_OF_CODE[min((word >> 10) & 7, 4)]))
    return {"records": recs[:n], "cand_index": cand_index[:n], "cands": cands, "allele_bytes": pool[:nb], "alleles": pairs, "info": info[:n],
            "venn_a": venn_a[:len(ra)], "venn_b": venn_b[:len(rb)], "n_out": (n, nc, nb)}


def venn_combine(a, b, options=None, comparison_case=-1):
    """pisces_hip_venn_combine: ConsensusBuilder.CombineVariants for one pair of rows (either may be None); comparison_case < 0 asks
    GetComparisonCase.  Returns (row, info, (VariantA.VariantQscore, VariantB.VariantQscore) as the call leaves them)."""
    opts = options if options is not None else venn_options()
    rows = [None if r is None else np.ascontiguousarray(np.asarray(r, dtype=_abi.CALLED_ALLELE_DTYPE).reshape(1)) for r in (a, b)]
    row = np.zeros(1, dtype=_abi.CALLED_ALLELE_DTYPE)
    info = _abi.PiscesConsensusInfo()
    vq = (C.c_int32 * 2)()
    _check(None, lib.pisces_hip_venn_combine(C.byref(opts), _address(rows[0]), _address(rows[1]), int(comparison_case), row.ctypes.data, C.byref(info), vq))
    return row[0], info, (int(vq[0]), int(vq[1]))


_CIGAR_RE = None


def exact_span_direction(cs, ce, cigar, directions, preceding, trailing, is_insertion=False):
    """pisces_hip_exact_span_direction for one read's coverage summary: cigar a string ("5M4I4M") or [(op, length)], directions the
    reference's direction string ("2F:9S:2R") or [(DIR_*, length)].  Returns 0 / 1 / 2, None when the read does not span [preceding,
    trailing]; raises where the reference throws (-2) or would index out of bounds (-3: runs longer than the read)."""
    global _CIGAR_RE
    if isinstance(cigar, str):
        import re
        _CIGAR_RE = _CIGAR_RE or re.compile(r"(\d+)([A-Za-z=])")
        cigar = [(m.group(2), int(m.group(1))) for m in _CIGAR_RE.finditer(cigar)]
    if isinstance(directions, str):
        directions = [("FRS".index(tok[-1]), int(tok[:-1])) for tok in directions.split(":") if tok]
    ops = np.array([ord(o) if isinstance(o, str) else int(o) for o, _ in cigar], dtype=np.uint8)
    lens = np.array([n for _, n in cigar], dtype=np.uint32)
    rt = np.array([d for d, _ in directions], dtype=np.uint8)
    rl = np.array([n for _, n in directions], dtype=np.uint32)
    rc = lib.pisces_hip_exact_span_direction(int(cs), int(ce), ops.ctypes.data, lens.ctypes.data, len(ops), rt.ctypes.data, rl.ctypes.data, len(rt),
                                             int(preceding), int(trailing), int(bool(is_insertion)))
    if rc == -1:
        return None
    if rc == -2:
        raise PiscesHipError(_abi.E_INVALID_ARG, "exact_span_direction: Invalid indices -1--1 (the reference throws InvalidDataException)")
    if rc < 0:
        raise PiscesHipError(_abi.E_INVALID_ARG, "exact_span_direction: arguments the reference would index out of bounds with: direction runs longer than "
                                                 "the CIGAR's read span, a direction above 2, or a missing array")
    return rc


def new_pad_state():
    """Cursors of a VCF writer + RegionMapper pair at the start of a chromosome (PiscesVcfPadState)."""
    return _abi.PiscesVcfPadState(0, 0, -1)


def vcf_pad_plan(records, intervals, state, finish=False, crush=False):
    """pisces_hip_vcf_pad_plan: what format_vcf(..., pad=dict(state=state, intervals=intervals, finish=finish)) would do without
    writing a line — (no-call rows, lines, the PiscesVcfPadState afterwards).  `state` is left as it is.  Raises PiscesHipError with
    E_UNSUPPORTED for rows in descending order or a state the formatter does not produce (the formatter itself still takes those)."""
    recs = np.ascontiguousarray(records, dtype=_abi.CALLED_ALLELE_DTYPE)
    iv = np.asarray(intervals, dtype=np.int32).reshape(-1, 2)
    starts, ends = np.ascontiguousarray(iv[:, 0]), np.ascontiguousarray(iv[:, 1])
    pads, lines, out = C.c_int64(0), C.c_int64(0), _abi.PiscesVcfPadState()
    rc = lib.pisces_hip_vcf_pad_plan(recs.ctypes.data if len(recs) else None, len(recs), int(bool(crush)), starts.ctypes.data if len(iv) else None,
                                     ends.ctypes.data if len(iv) else None, len(iv), C.byref(state), int(bool(finish)), C.byref(pads), C.byref(lines),
                                     C.byref(out))
    if rc != 0:
        raise PiscesHipError(int(rc), "vcf_pad_plan: intervals that are not positive, sorted and disjoint" if rc == _abi.E_INVALID_ARG else
                             "vcf_pad_plan: rows in descending order, or a state the formatter does not produce")
    return pads.value, lines.value, out


def format_vcf(chrom, records, vcf_config=None, alleles=None, pad=None, posteriors=None, **overrides):
    """VCF body lines of `records` (pisces_hip_format_vcf[_padded][_ex]).  posteriors: the POSTERIORS_DTYPE array Posteriors() returned for
    these rows (the GP column of PloidyModel.DiploidByAdaptiveGT), None = none.  alleles: the (ref, alt) string pairs CallWithAlleles returned, needed
    for insertion / deletion / MNV rows; vcf_config: _abi.PiscesVcfConfig or None for the defaults (+ field overrides, e.g. crush=1,
    indel_repeat_filter=8 for the R8 name of FILTER_INDEL_REPEAT_LENGTH).
    pad: dict(state=new_pad_state(), reference=bytes, intervals=[(start, end), ...], finish=bool) adds RegionMapper's no-call rows for
    uncovered interval positions; the state object is advanced in place."""
    cfg = vcf_config
    if cfg is None:
        cfg = _abi.PiscesVcfConfig()
        _check(None, lib.pisces_hip_vcf_default_config(C.byref(cfg)))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    recs = np.ascontiguousarray(records)
    n = len(recs)
    gp = None
    if posteriors is not None:
        gp = np.ascontiguousarray(posteriors, dtype=_abi.POSTERIORS_DTYPE)
        if len(gp) != n:
            raise ValueError("format_vcf: posteriors must have one entry per record")
    idx = cands = pool_arr = None
    if alleles is not None:
        idx_l, cand_l, pool = [], [], bytearray()
        for (r, a) in alleles:
            if len(r) == 1 and len(a) == 1:
                idx_l.append(-1)
                continue
            c = _abi.PiscesCandidate()
            c.ref_len, c.alt_len, c.allele_offset = len(r), len(a), len(pool)
            pool += r.encode() + a.encode()
            idx_l.append(len(cand_l))
            cand_l.append(c)
        idx = np.array(idx_l, dtype=np.int32)
        cands = (_abi.PiscesCandidate * max(len(cand_l), 1))(*cand_l)
        pool_arr = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy()
    refa = starts = ends = state = None
    n_iv = finish = 0
    if pad is not None:
        refa = np.ascontiguousarray(np.frombuffer(pad["reference"], dtype=np.uint8) if isinstance(pad["reference"], (bytes, bytearray))
                                    else pad["reference"], np.uint8)
        starts = np.array([a for a, _ in pad["intervals"]], dtype=np.int32)
        ends = np.array([b for _, b in pad["intervals"]], dtype=np.int32)
        n_iv, finish, state = len(starts), int(bool(pad.get("finish"))), pad["state"]
    pad_rows = 0
    if pad is not None and n_iv:   # the call's own no-call rows where the plan gives them, every interval position where it does not
        pad_rows = int((ends.astype(np.int64) - starts + 1).sum())
        planned, planned_lines = C.c_int64(0), C.c_int64(0)
        if lib.pisces_hip_vcf_pad_plan(recs.ctypes.data if n else None, n, int(cfg.crush), starts.ctypes.data, ends.ctypes.data, n_iv,
                                       C.byref(state), finish, C.byref(planned), C.byref(planned_lines), None) == 0:
            pad_rows = planned.value
    cap = 256 * max(n, 1) + (128 + len(chrom)) * pad_rows
    while True:
        buf = C.create_string_buffer(max(cap, 1))
        need = lib.pisces_hip_format_vcf_padded_ex(
            C.byref(cfg), chrom.encode(), recs.ctypes.data if n else None, n, idx.ctypes.data if idx is not None else None, cands,
            pool_arr.ctypes.data if pool_arr is not None else None, refa.ctypes.data if refa is not None else None,
            refa.size if refa is not None else 0, starts.ctypes.data if n_iv else None, ends.ctypes.data if n_iv else None, n_iv,
            C.byref(state) if state is not None else None, finish, buf, cap, gp.ctypes.data if gp is not None and n else None)
        if need < 0:
            raise PiscesHipError(int(need), "format_vcf failed")
        if need <= cap:
            return buf.raw[:need].decode()
        cap = int(need)


def find_indel_candidates(batch, ref, min_base_call_quality=20):
    """Host finder for insertions / deletions (pisces_hip_find_indel_candidates): list of dicts in read order."""
    return find_candidates(batch, ref, min_base_call_quality, snvs_and_mnvs=False)


def bgzf_scan(file_bytes):
    """pisces_hip_bgzf_scan: the BGZF block table of the file bytes (host); returns (ctypes array of PiscesBgzfBlock, inflated size)."""
    data = file_bytes if isinstance(file_bytes, np.ndarray) else np.frombuffer(bytes(file_bytes), dtype=np.uint8)
    total = C.c_int64(0)
    n = lib.pisces_hip_bgzf_scan(data.ctypes.data, data.size, None, 0, C.byref(total))
    if n < 0:
        raise PiscesHipError(int(n), "not a chain of BGZF blocks")
    blocks = (_abi.PiscesBgzfBlock * max(int(n), 1))()
    n2 = lib.pisces_hip_bgzf_scan(data.ctypes.data, data.size, blocks, n, C.byref(total))
    assert n2 == n
    return (_abi.PiscesBgzfBlock * int(n)).from_buffer(blocks) if n else (_abi.PiscesBgzfBlock * 0)(), int(total.value)


def _candidate_dicts(cands, pool, n):
    out = []
    for i in range(n):
        c = cands[i]
        o = c.allele_offset
        out.append({"position": c.position, "category": c.category, "ref": bytes(pool[o: o + c.ref_len]).decode("latin-1"),   # (inserted bases are whatever bytes the read holds)
                    "alt": bytes(pool[o + c.ref_len: o + c.ref_len + c.alt_len]).decode("latin-1"),
                    "support_by_dir": list(c.support_by_dir), "well_anchored_by_dir": list(c.well_anchored_by_dir),
                    "open_left": bool(c.open_left), "open_right": bool(c.open_right)})
    return out


def find_candidates(batch, ref, min_base_call_quality=20, snvs_and_mnvs=True, call_mnvs=False, max_mnv_length=3, max_gap_between_mnv=1):
    """The host finder (pisces_hip_find_candidates): insertions / deletions, and with snvs_and_mnvs the SNV / MNV candidates of the
    M operations; list of dicts in read order."""
    refa = np.ascontiguousarray(np.frombuffer(ref, dtype=np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, np.uint8)
    cap, pool_cap = 4096, 1 << 18
    while True:
        cands = (_abi.PiscesCandidate * cap)()
        pool = np.zeros(pool_cap, dtype=np.uint8)
        nb = C.c_int64(0)
        n = lib.pisces_hip_find_candidates(C.byref(batch.c), refa.ctypes.data, refa.size, min_base_call_quality, int(snvs_and_mnvs),
                                           int(call_mnvs), max_mnv_length, max_gap_between_mnv, cands, cap, pool.ctypes.data, pool_cap,
                                           C.byref(nb))
        if n == _abi.E_BUFFER_TOO_SMALL:
            cap *= 4
            pool_cap = max(pool_cap * 4, int(nb.value))
            continue
        if n < 0:
            raise PiscesHipError(int(n), "find_candidates failed")
        return _candidate_dicts(cands, pool, n)


# ---- Scylla's read pass (pisces_hip_vead_*) ---------------------------------------------------------------------------------------------
def vead_options(**overrides):
    """PiscesVeadOptions with Scylla's defaults (pisces_hip_vead_default_options), fields overridden by name."""
    opts = _abi.PiscesVeadOptions()
    _check(None, lib.pisces_hip_vead_default_options(C.byref(opts)))
    for k, v in overrides.items():
        if not hasattr(opts, k):
            raise AttributeError(f"PiscesVeadOptions has no field {k!r}")
        setattr(opts, k, v)
    return opts


def vead_sites(sites):
    """[(position, ref, alt), ...] (alleles as bytes or str) as (VEAD_SITE_DTYPE rows, the allele bytes they point into).  A pair that
    vead_sites made is passed through."""
    if isinstance(sites, tuple) and len(sites) == 2 and getattr(sites[0], "dtype", None) == _abi.VEAD_SITE_DTYPE:
        return sites
    rows = np.zeros(len(sites), dtype=_abi.VEAD_SITE_DTYPE)
    pool = bytearray()
    for i, (position, ref, alt) in enumerate(sites):
        ref = ref.encode() if isinstance(ref, str) else bytes(ref)
        alt = alt.encode() if isinstance(alt, str) else bytes(alt)
        rows[i] = (position, len(ref), len(alt), len(pool))
        pool += ref + alt
    alleles = np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy()[:len(pool)]
    return rows, alleles


def _vead_neighborhoods(neighborhoods):
    nb = np.zeros(len(neighborhoods), dtype=_abi.VEAD_NEIGHBORHOOD_DTYPE)
    for i, (b, e) in enumerate(neighborhoods):
        nb[i] = (b, e)
    return nb


def vead_out(groups, states, info, n_out, group_capacity, state_capacity):
    """PiscesVeadOut: where the groups go (torch tensors, numpy arrays, ctypes arrays or raw addresses; the caller keeps them alive)."""
    o = _abi.PiscesVeadOut()
    o.groups, o.states, o.info, o.n_out = _address(groups), _address(states), _address(info), _address(n_out)
    o.group_capacity, o.state_capacity = int(group_capacity), int(state_capacity)
    return o


def vead_site_states(position, cigar, bases, quals, sites, options=None):
    """pisces_hip_vead_site_states: what ONE read (Read.Position 1-based, cigar [(op char, length), ...], bases, quals) says about each of
    `sites` (vead_sites input).  Returns (states uint8[n_sites], sites in range)."""
    opts = options if options is not None else vead_options()
    rows, alleles = vead_sites(sites)
    ops = np.array([ord(o) if isinstance(o, str) else int(o) for o, _ in cigar], dtype=np.uint8)
    lens = np.array([int(n) for _, n in cigar], dtype=np.uint32)
    b = np.frombuffer(bases.encode() if isinstance(bases, str) else bytes(bases), dtype=np.uint8)
    q = np.ascontiguousarray(quals, dtype=np.uint8)
    states = np.zeros(max(len(rows), 1), dtype=np.uint8)
    found = C.c_int32(0)
    _check(None, lib.pisces_hip_vead_site_states(C.byref(opts), int(position), ops.ctypes.data, lens.ctypes.data, len(ops), b.ctypes.data, q.ctypes.data,
                                                 len(b), rows.ctypes.data, len(rows), alleles.ctypes.data, alleles.size, states.ctypes.data, C.byref(found)))
    return states[:len(rows)], int(found.value)


def vead_neighborhood_info(sites):
    """pisces_hip_vead_neighborhood_info: (first, last_with_look_ahead, soft_clip_end_before, soft_clip_pos_after) of a site list in the
    caller's order."""
    rows, _ = vead_sites(sites)
    info = _abi.PiscesVeadNeighborhoodInfo()
    _check(None, lib.pisces_hip_vead_neighborhood_info(rows.ctypes.data, len(rows), C.byref(info)))
    return info.first, info.last_with_look_ahead, info.soft_clip_end_before, info.soft_clip_pos_after


def vead_groups(batch, sites, neighborhoods, options=None, capacities=None):
    """pisces_hip_vead_groups: the vead groups of every neighbourhood over a HOST batch (a mapping or an object with the PiscesReadBatch
    field names as numpy arrays).  Returns {groups (VEAD_GROUP_DTYPE), states (uint8), info (VEAD_INFO_DTYPE), n_out}.  capacities: (groups, state
    bytes); by default the call is repeated with the sizes it reports."""
    opts = options if options is not None else vead_options()
    rows, alleles = vead_sites(sites)
    nb = _vead_neighborhoods(neighborhoods)
    get = (lambda k: batch[k]) if hasattr(batch, "__getitem__") else (lambda k: getattr(batch, k))
    arrays = {k: np.ascontiguousarray(get(k), dtype=dt) for k, dt in (("position", np.int32), ("cigar_offset", np.int32), ("cigar_op", np.uint8),
                                                                      ("cigar_len", np.uint32), ("seq_offset", np.int32), ("bases", np.uint8), ("quals", np.uint8))}
    c = _abi.PiscesReadBatch()
    c.n_reads = len(arrays["position"])
    for k, a in arrays.items():
        setattr(c, k, C.cast(C.c_void_p(a.ctypes.data if a.size else (np.zeros(1, a.dtype)).ctypes.data), type(getattr(c, k))))
    caps = capacities if capacities is not None else (0, 0)
    while True:
        groups = np.zeros(max(caps[0], 1), dtype=_abi.VEAD_GROUP_DTYPE)
        states = np.zeros(max(caps[1], 1), dtype=np.uint8)
        info = np.zeros(max(len(nb), 1), dtype=_abi.VEAD_INFO_DTYPE)
        n_out = np.zeros(3, dtype=np.int64)
        out = vead_out(groups, states, info, n_out, caps[0], caps[1])
        rc = lib.pisces_hip_vead_groups(C.byref(opts), C.byref(c), rows.ctypes.data, len(rows), alleles.ctypes.data, alleles.size, nb.ctypes.data, len(nb),
                                        C.byref(out))
        if rc == _abi.E_BUFFER_TOO_SMALL and capacities is None:
            caps = (int(n_out[0]), int(n_out[1]))
            continue
        if rc != 0:
            err = PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode())
            err.n_out = tuple(int(v) for v in n_out)
            raise err
        return {"groups": groups[:int(n_out[0])], "states": states[:int(n_out[1])], "info": info[:len(nb)], "n_out": tuple(int(v) for v in n_out)}


# ---- Scylla's neighbourhoods (pisces_hip_nbhd_*) ----------------------------------------------------------------------------------------
def nbhd_criteria(**overrides):
    """PiscesNbhdCriteria with Scylla's defaults (pisces_hip_nbhd_default_criteria), fields overridden by name."""
    crit = _abi.PiscesNbhdCriteria()
    _check(None, lib.pisces_hip_nbhd_default_criteria(C.byref(crit)))
    for k, v in overrides.items():
        if not hasattr(crit, k):
            raise AttributeError(f"PiscesNbhdCriteria has no field {k!r}")
        setattr(crit, k, int(v))
    return crit


def nbhd_out(sites, alleles, site_row, site_original, neighbourhoods, info, ref_bytes, n_out, nbhd_capacity, site_capacity, allele_capacity, ref_capacity,
             row_class=None):
    """PiscesNbhdOut: where the tables go (torch tensors, numpy arrays, ctypes arrays or raw addresses; the caller keeps them alive)."""
    o = _abi.PiscesNbhdOut()
    o.sites, o.alleles, o.site_row, o.site_original = _address(sites), _address(alleles), _address(site_row), _address(site_original)
    o.neighbourhoods, o.info, o.ref_bytes, o.row_class, o.n_out = _address(neighbourhoods), _address(info), _address(ref_bytes), _address(row_class), _address(n_out)
    o.nbhd_capacity, o.site_capacity, o.allele_capacity, o.ref_capacity = int(nbhd_capacity), int(site_capacity), int(allele_capacity), int(ref_capacity)
    return o


def _nbhd_error_word(counts):
    """the PiscesHipError of an n_out that holds an error word"""
    if counts[0] == _abi.E_INVALID_ARG and counts[1] == 0:
        text = f"nbhd_build_device: the rows are not sorted by position at row {counts[2]}"
    elif counts[0] == _abi.E_INVALID_ARG:
        text = f"nbhd_build_device: row {counts[2]} is an insertion, deletion or MNV without a candidate to take its alleles from"
    else:
        text = "nbhd_build_device: more than 2^31 - 1 allele or reference bytes"
    err = PiscesHipError(counts[0], text)
    err.n_out = tuple(counts)
    return err


def _nbhd_result(raw, counts, n_rows):
    """the tables cut to their counts, from byte (or typed) arrays"""
    k, ns, nb, nr = counts[:4]
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return {"sites": as_bytes(raw["sites"])[:ns * 16].view(_abi.VEAD_SITE_DTYPE).copy(), "alleles": as_bytes(raw["alleles"])[:nb].copy(),
            "site_row": as_bytes(raw["site_row"])[:ns * 4].view(np.int32).copy(), "site_original": as_bytes(raw["site_original"])[:ns * 4].view(np.int32).copy(),
            "neighbourhoods": as_bytes(raw["neighbourhoods"])[:k * 8].view(_abi.VEAD_NEIGHBORHOOD_DTYPE).copy(),
            "info": as_bytes(raw["info"])[:k * 48].view(_abi.NBHD_INFO_DTYPE).copy(), "ref_bytes": as_bytes(raw["ref_bytes"])[:nr].copy(),
            "row_class": as_bytes(raw["row_class"])[:n_rows].copy(), "n_out": tuple(counts)}


def nbhd_build(records, alleles=None, criteria=None, reference=None, capacities=None, count=None):
    """pisces_hip_nbhd_build: Scylla's neighbourhoods over host rows (a CALLED_ALLELE_DTYPE array of one chromosome, sorted by position);
    alleles: format_vcf's (ref, alt) pairs when there are insertion / deletion / MNV rows; reference: the chromosome's bases (position p at
    [p - 1]) or None; count: a row count below len(records).  Returns {sites (VEAD_SITE_DTYPE), alleles, site_row, site_original,
    neighbourhoods (VEAD_NEIGHBORHOOD_DTYPE), info (NBHD_INFO_DTYPE), ref_bytes, row_class, n_out}.  capacities: (neighbourhoods, sites,
    allele bytes, reference bytes) to offer; by default the call is repeated with the sizes it reports.  A refusal raises PiscesHipError
    whose n_out attribute holds the six words."""
    crit = criteria if criteria is not None else nbhd_criteria()
    recs = np.ascontiguousarray(records, dtype=_abi.CALLED_ALLELE_DTYPE)
    table = candidate_table(recs, alleles) if alleles is not None else (None, None, None)
    count_word = None if count is None else np.array([count], dtype=np.int32)
    rows = venn_rows(recs if len(recs) else None, len(recs), count_word, *table)
    if reference is not None:
        reference = np.frombuffer(reference.encode() if isinstance(reference, str) else bytes(reference), dtype=np.uint8) if not isinstance(reference, np.ndarray) \
            else np.ascontiguousarray(reference, np.uint8)
    caps = tuple(capacities) if capacities is not None else (0, 0, 0, 0)
    while True:
        raw = {"sites": np.zeros(max(caps[1], 1), dtype=_abi.VEAD_SITE_DTYPE), "alleles": np.zeros(max(caps[2], 1), np.uint8),
               "site_row": np.zeros(max(caps[1], 1), np.int32), "site_original": np.zeros(max(caps[1], 1), np.int32),
               "neighbourhoods": np.zeros(max(caps[0], 1), dtype=_abi.VEAD_NEIGHBORHOOD_DTYPE), "info": np.zeros(max(caps[0], 1), dtype=_abi.NBHD_INFO_DTYPE),
               "ref_bytes": np.zeros(max(caps[3], 1), np.uint8), "row_class": np.full(max(len(recs), 1), 255, np.uint8)}
        n_out = np.zeros(6, dtype=np.int64)
        out = nbhd_out(raw["sites"], raw["alleles"], raw["site_row"], raw["site_original"], raw["neighbourhoods"], raw["info"], raw["ref_bytes"], n_out, *caps,
                       row_class=raw["row_class"])
        rc = lib.pisces_hip_nbhd_build(C.byref(crit), C.byref(rows), None if reference is None else reference.ctypes.data,
                                       0 if reference is None else reference.size, C.byref(out))
        if rc == _abi.E_BUFFER_TOO_SMALL and capacities is None:
            caps = tuple(int(v) for v in n_out[:4])
            continue
        if rc != 0:
            err = PiscesHipError(rc, (lib.pisces_hip_last_error(None) or b"").decode())
            err.n_out = tuple(int(v) for v in n_out)
            raise err
        return _nbhd_result(raw, [int(v) for v in n_out], len(recs) if count is None else max(0, min(len(recs), int(count))))
