"""Host-side handle on the HIP hot path (one Engine per GPU).

Mirrors the stages of LongSom's SNV chain as methods:
  set_barcodes   <- meta_to_dict / split_bam routing   (scripts/PreProcessing/SplitBamCellTypes.py:16-36,83-90)
  load_reads     <- reading the BAM                     (scripts/SNVCalling/BaseCellCounter.py:190-191)
  pileup_count   <- run_interval over all windows       (BaseCellCounter.py:182-320)
  call_step1     <- merge + variant_calling_step1       (MergeBaseCellCounts.py:116-204, BaseCellCalling.step1.py:19-476)
"""
import contextlib
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import CallParams, CountParams, CountStats, Reads, ROW_WORDS


@dataclass
class ReadRecords:
    """Pre-decoded read-record arrays (SoA form of a coordinate-sorted BAM; include/longsom_hip.h)."""
    read_tid: np.ndarray      # int32 [R]
    read_pos: np.ndarray      # int32 [R]
    read_flag: np.ndarray     # uint16 [R]
    read_mapq: np.ndarray     # uint8 [R]
    read_cb: np.ndarray       # int32 [R]  dense barcode id, -1 = none
    seg_read: np.ndarray      # uint32 [S]
    seg_start: np.ndarray     # int32 [S]
    seg_len: np.ndarray       # int32 [S]
    seg_ev_off: np.ndarray    # int64 [S]
    events: np.ndarray        # uint16 [E]  LSG_EVENT: 0x0800 | sym << 8 | qual, 0 for 'NA'
    read_names: Optional[List[str]] = field(default=None, repr=False)

    _SPEC = (("read_tid", np.int32), ("read_pos", np.int32), ("read_flag", np.uint16), ("read_mapq", np.uint8),
             ("read_cb", np.int32), ("seg_read", np.uint32), ("seg_start", np.int32), ("seg_len", np.int32),
             ("seg_ev_off", np.int64), ("events", np.uint16))

    def __post_init__(self):
        for name, dt in self._SPEC:
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=dt))
        assert len(self.read_pos) == len(self.read_tid) == len(self.read_flag) == len(self.read_mapq) == len(self.read_cb)
        assert len(self.seg_start) == len(self.seg_read) == len(self.seg_len) == len(self.seg_ev_off)

    @classmethod
    def empty(cls) -> "ReadRecords":
        return cls(*[np.zeros(0, dt) for _, dt in cls._SPEC])

    @property
    def n_reads(self): return len(self.read_tid)
    @property
    def n_segs(self): return len(self.seg_read)
    @property
    def n_events(self): return len(self.events)

    def subset(self, read_mask: np.ndarray) -> "ReadRecords":
        """Records of the reads selected by a boolean mask (events re-packed)."""
        read_mask = np.asarray(read_mask, dtype=bool)
        new_idx = np.cumsum(read_mask) - 1
        seg_keep = read_mask[self.seg_read]
        seg_len = self.seg_len[seg_keep]
        seg_off_old = self.seg_ev_off[seg_keep]
        seg_off_new = np.concatenate([[0], np.cumsum(seg_len)[:-1]]).astype(np.int64) if len(seg_len) else np.zeros(0, np.int64)
        if len(seg_len):
            idx = np.repeat(seg_off_old - seg_off_new, seg_len) + np.arange(int(seg_len.sum()), dtype=np.int64)
            events = self.events[idx]
        else:
            events = np.zeros(0, np.uint16)
        names = [n for n, m in zip(self.read_names, read_mask) if m] if self.read_names is not None else None
        return ReadRecords(self.read_tid[read_mask], self.read_pos[read_mask], self.read_flag[read_mask],
                           self.read_mapq[read_mask], self.read_cb[read_mask],
                           new_idx[self.seg_read[seg_keep]].astype(np.uint32), self.seg_start[seg_keep], seg_len,
                           seg_off_new, events, names)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


class Engine:
    """One liblongsom_hip handle.  Raises if the HIP library or a GPU is missing (no CPU fallback)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, keep_reads: bool = False):
        """keep_reads: loads also keep the compact events beside the tile store, so that reads_to_host() can return them
        (tests, sampling for the CPU baseline); the product paths leave it off — the store is the only resident copy."""
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.lsg_create(int(device), C.byref(h)), "lsg_create")
        self._h = h
        self.device = device
        self.n_ct = 0
        self.n_contigs = 0
        self.contig_len = None
        self.pileup_window = 50000
        self._bbfit_cap = 0
        self._load_settings = {"load_filter": (0, 0, 0), "count_at_load": None, "store_policy": 0, "keep_unlisted": False,      # the library's defaults
                               "split_filters": (-1, -1, 0)}
        if stream is not None:
            self.set_stream(stream)
        if keep_reads:
            self.set_keep_reads(True)

    def set_load_filter(self, min_mq: int = 0, flag_exclude: int = 0, ignore_orphans: int = 0):
        """Reads failing these are not stored by the next loads (what SplitBamCellTypes.py:110-113 does before BaseCellCounter sees the
        BAM); later counts must be at least as strict.  Default: no filter (lsg_set_load_filter)."""
        _lib.check(self._lib.lsg_set_load_filter(self._h, int(min_mq), int(flag_exclude), int(ignore_orphans)), "lsg_set_load_filter")
        self._load_settings["load_filter"] = (int(min_mq), int(flag_exclude), int(ignore_orphans))

    LAYOUT_COMPACT, LAYOUT_PHASED = 0, 1

    def set_events_layout(self, layout: int = 0):
        """what the caller promises about the events of the next load_reads calls: LAYOUT_PHASED = every segment at an offset congruent to its
        reference start modulo 128 (lsg_set_events_layout; checked by the load, which falls back by itself)"""
        _lib.check(self._lib.lsg_set_events_layout(self._h, int(layout)), "lsg_set_events_layout")

    def set_pileup_window(self, window: int = 50000):
        """the reference's pileup windows (BaseCellCounter.py --bin): the loads that follow cut their entries at the window edges, the depth
        cap of a count is replayed per window (lsg_set_pileup_window)"""
        _lib.check(self._lib.lsg_set_pileup_window(self._h, int(window)), "lsg_set_pileup_window")
        self.pileup_window = int(window)

    def set_count_at_load(self, params=None):
        """The loads that follow also make the first count under `params` (a CountParams), in the pass that builds the store; the
        first pileup_count(params) after such a load returns that count without another pass.  None switches it off
        (lsg_set_count_at_load).  Barcodes, references and region must be set before the load."""
        import ctypes as C
        _lib.check(self._lib.lsg_set_count_at_load(self._h, C.byref(params) if params is not None else None), "lsg_set_count_at_load")
        self._load_settings["count_at_load"] = params

    def set_keep_unlisted(self, on: bool):
        """The BAM loads that follow keep reads without a listed barcode (cb = -1): never counted, but part of the buffer the per-cell
        genotyping's pileup of the unsplit BAM fills (HCCVSingleCellGenotype.py:121-122; lsg_set_keep_unlisted)."""
        _lib.check(self._lib.lsg_set_keep_unlisted(self._h, 1 if on else 0), "lsg_set_keep_unlisted")
        self._load_settings["keep_unlisted"] = bool(on)

    def set_split_filters(self, filters=None):
        """SplitBam's --max_nM / --max_NH / --n_trim (a hostio.SplitFilters; None: off) for the BAM loads that follow: a read with an nM / NH
        reason is never counted, a passing read's trim window is stored with quality 0 (lsg_set_split_filters)."""
        args = (-1, -1, 0) if filters is None else tuple(filters.args())
        _lib.check(self._lib.lsg_set_split_filters(self._h, *[int(x) for x in args]), "lsg_set_split_filters")
        self._load_settings["split_filters"] = args

    def split_reasons(self):
        """(n[18], first_ordinal[18]) of the last BAM load: records per filter reason and the smallest record ordinal of each (-1: none);
        hostio.split_report turns them into the report's columns (lsg_get_split_reasons)."""
        n = np.zeros(18, np.int64); first = np.zeros(18, np.int64)
        _lib.check(self._lib.lsg_get_split_reasons(self._h, _ptr(n), _ptr(first)), "lsg_get_split_reasons")
        return n, first

    STORE_KEEP, STORE_SKIP_WHEN_COUNTED = 0, 1

    def set_store_policy(self, policy: int):
        """STORE_SKIP_WHEN_COUNTED: a load that makes its count in its own pass (set_count_at_load) counts straight from the caller's
        events and keeps no tile store - for a BAM that is counted once (the reference's BaseCellCounter rule); anything that needs
        the store afterwards (another count, genotype_cells) raises until reads are loaded again.  STORE_KEEP is the default
        (lsg_set_store_policy)."""
        _lib.check(self._lib.lsg_set_store_policy(self._h, int(policy)), "lsg_set_store_policy")
        self._load_settings["store_policy"] = int(policy)

    def load_settings(self) -> dict:
        """what the next loads will do, as this wrapper last set it (load filter, count at load, store policy, unlisted reads, split filters):
        a caller that changes them for one load puts them back with restore_load_settings (or lets `loading` do both)"""
        return dict(self._load_settings)

    @contextlib.contextmanager
    def loading(self, count=None, keep_store: bool = True, keep_unlisted: Optional[bool] = None, filters=None):
        """The load settings of the loads made inside the `with` block; the ones they replace are put back when it ends, on an error too.
        count: the loads also make that count (set_count_at_load; None: no count at load).  keep_store=False with a count: it is the only
        count anybody will ask of these reads - the loads keep no tile store (STORE_SKIP_WHEN_COUNTED) and, unless they keep unlisted
        reads, do not store what the count's own read filters refuse (set_load_filter, what SplitBamCellTypes.py:110-113 does to the BAM a
        rule counts: every stored read is then admitted and the load sorts keys alone).  keep_unlisted: set_keep_unlisted (None: as it
        is).  filters: set_split_filters (a hostio.SplitFilters; None: off)."""
        saved = self.load_settings()
        try:
            if keep_unlisted is not None:
                self.set_keep_unlisted(keep_unlisted)
            self.set_split_filters(filters)
            once = count is not None and not keep_store
            self.set_count_at_load(count)
            self.set_store_policy(self.STORE_SKIP_WHEN_COUNTED if once else self.STORE_KEEP)
            if once and not self._load_settings["keep_unlisted"]:
                self.set_load_filter(count.min_mq, count.flag_exclude, count.ignore_orphans)
            yield self
        finally:
            self.restore_load_settings(saved)

    def restore_load_settings(self, saved: dict):
        self.set_load_filter(*saved["load_filter"])
        self.set_count_at_load(saved["count_at_load"])
        self.set_store_policy(saved["store_policy"])
        self.set_keep_unlisted(saved["keep_unlisted"])
        if "split_filters" in saved:
            _lib.check(self._lib.lsg_set_split_filters(self._h, *[int(x) for x in saved["split_filters"]]), "lsg_set_split_filters")
            self._load_settings["split_filters"] = tuple(saved["split_filters"])

    def unload_reads(self):
        """give the device memory of the resident load (reads, store, rows, call records, cached temporaries) back: lsg_unload_reads"""
        _lib.check(self._lib.lsg_unload_reads(self._h), "lsg_unload_reads")
        self._n_rows = [0] * max(1, self.n_ct)
        self._n_sites = 0

    def set_keep_reads(self, keep: bool):
        _lib.check(self._lib.lsg_set_keep_reads(self._h, 1 if keep else 0), "lsg_set_keep_reads")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self): return self
    def __exit__(self, *exc): self.close()

    # ---- inputs ------------------------------------------------------------------------------
    def set_stream(self, hip_stream: int):
        _lib.check(self._lib.lsg_set_stream(self._h, C.c_void_p(hip_stream)), "lsg_set_stream")

    def synchronize(self):
        _lib.check(self._lib.lsg_synchronize(self._h), "lsg_synchronize")

    def set_contigs(self, lengths):
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        _lib.check(self._lib.lsg_set_contigs(self._h, len(lengths), _ptr(lengths)), "lsg_set_contigs")
        self.n_contigs = len(lengths)
        self.contig_len = lengths.copy()

    def load_reference(self, tid: int, bases, on_device: bool = False, length: Optional[int] = None):
        """bases: uint8 array of upper-cased ASCII bases (host), or a device pointer + length."""
        if on_device:
            _lib.check(self._lib.lsg_load_reference(self._h, tid, C.c_void_p(int(bases)), int(length), 1), "lsg_load_reference")
            return
        if isinstance(bases, (bytes, bytearray, str)):
            bases = np.frombuffer(bases.encode() if isinstance(bases, str) else bytes(bases), dtype=np.uint8)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        _lib.check(self._lib.lsg_load_reference(self._h, tid, _ptr(bases) if bases.size else C.c_void_p(bases.ctypes.data), len(bases), 0),
                   "lsg_load_reference")

    def set_barcodes(self, celltype_of, n_celltypes: int):
        ct = np.ascontiguousarray(celltype_of, dtype=np.uint8)
        # (a table identical to the one the handle holds is left alone by the library itself: setting one drops the resident count, and the one
        # a load made under set_count_at_load would be counted again)
        _lib.check(self._lib.lsg_set_barcodes(self._h, _ptr(ct), len(ct), int(n_celltypes)), "lsg_set_barcodes")
        self.n_ct = int(n_celltypes)
        self.n_cb = len(ct)

    def load_reads(self, rec: ReadRecords):
        """Builds the tile store of these reads on the device (lsg_load_reads); the arrays are free again on return."""
        r = Reads(rec.n_reads, rec.n_segs, rec.n_events, *[_ptr(getattr(rec, n)) for n, _ in ReadRecords._SPEC], 0)
        _lib.check(self._lib.lsg_load_reads(self._h, C.byref(r)), "lsg_load_reads")

    def load_reads_device(self, n_reads, n_segs, n_events, ptrs: dict):
        """ptrs: name -> device pointer (int) for every array of ReadRecords._SPEC; arrays stay owned by the caller."""
        r = Reads(n_reads, n_segs, n_events, *[C.c_void_p(int(ptrs[n])) for n, _ in ReadRecords._SPEC], 1)
        _lib.check(self._lib.lsg_load_reads(self._h, C.byref(r)), "lsg_load_reads")

    def load_reads_struct(self, reads: Reads):
        """lsg_load_reads of a ready lsg_reads (e.g. what synth_generate returned)"""
        _lib.check(self._lib.lsg_load_reads(self._h, C.byref(reads)), "lsg_load_reads")

    def load_bam(self, path: str, barcodes, min_mapq: int = 60, first_record_offset: Optional[int] = None, legacy_del_merge: Optional[bool] = None):
        """Device-side ingest (lsg_load_bam): the BAM's bytes go to the GPU as they are; BGZF inflate, record decode, CB lookup, SplitBam's
        counters and the CIGAR walk run there and the tile store is built from the device arrays.  Set the contigs (hostio.bam_header)
        first.  Returns (info dict with the report counters and the phases' times, cb_pass, cb_low per dense barcode id).  Raises
        _lib.LsgError with rc -4 in its text ("straddle") for a BAM whose records are not aligned to its BGZF blocks: decode that one on
        the host (hostio.decode_bam)."""
        import mmap
        from . import hostio
        from ._lib import BamInfo
        if first_record_offset is None:
            first_record_offset = hostio.bam_header(path)[2]
        if legacy_del_merge is None:
            legacy_del_merge = bool(hostio.load().lsio_get_legacy_del_merge())
        joined = "\n".join(barcodes).encode()
        n_cb = len(barcodes)
        info = BamInfo()
        cb_pass = np.zeros(n_cb, np.int64); cb_low = np.zeros(n_cb, np.int64)
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                buf = np.frombuffer(mm, dtype=np.uint8)
                try:
                    _lib.check(self._lib.lsg_load_bam(self._h, C.c_void_p(buf.ctypes.data), size, int(first_record_offset), joined, n_cb, None, int(min_mapq),
                                                      1 if legacy_del_merge else 0, C.byref(info), _ptr(cb_pass), _ptr(cb_low), n_cb), "lsg_load_bam")
                finally:
                    del buf
        d = {k: getattr(info, k) for k, _ in BamInfo._fields_ if k != "pad_"}
        return d, cb_pass, cb_low

    def load_bam_range(self, slice_bytes: np.ndarray, first_record_offset: int, barcodes, min_mapq: int, count_lo_key: int, count_hi_key: int,
                       legacy_del_merge: Optional[bool] = None):
        """lsg_load_bam_range: a slice of whole BGZF blocks of a coordinate-sorted BAM (uint8 array, e.g. a view of a memory map), a record
        starting at first_record_offset of its first block; the counters and tallies take the records with (tid << 32 | pos) in
        [count_lo_key, count_hi_key).  Returns what load_bam returns; info["last_key"] = key of the slice's last complete record."""
        from . import hostio
        from ._lib import BamInfo
        if legacy_del_merge is None:
            legacy_del_merge = bool(hostio.load().lsio_get_legacy_del_merge())
        joined = "\n".join(barcodes).encode()
        n_cb = len(barcodes)
        info = BamInfo()
        cb_pass = np.zeros(n_cb, np.int64); cb_low = np.zeros(n_cb, np.int64)
        buf = np.ascontiguousarray(slice_bytes, dtype=np.uint8)
        _lib.check(self._lib.lsg_load_bam_range(self._h, C.c_void_p(buf.ctypes.data), len(buf), int(first_record_offset), joined, n_cb, None, int(min_mapq),
                                                1 if legacy_del_merge else 0, int(count_lo_key), int(count_hi_key), C.byref(info), _ptr(cb_pass), _ptr(cb_low), n_cb),
                   "lsg_load_bam_range")
        return {k: getattr(info, k) for k, _ in BamInfo._fields_ if k != "pad_"}, cb_pass, cb_low

    def set_region(self, tid_lo=0, pos_lo=0, tid_hi=None, pos_hi=0):
        """Count only columns in [(tid_lo,pos_lo), (tid_hi,pos_hi)) — window sharding across GPUs."""
        tid_hi = self.n_contigs if tid_hi is None else tid_hi
        _lib.check(self._lib.lsg_set_region(self._h, int(tid_lo), int(pos_lo), int(tid_hi), int(pos_hi)), "lsg_set_region")

    # ---- synthetic workload (bench / tests) -------------------------------------------------------
    def synth_reference(self, seed: int):
        _lib.check(self._lib.lsg_synth_reference(self._h, C.c_uint64(seed)), "lsg_synth_reference")

    def synth_reads(self, model):
        """model: longsom_amd.synth.SynthModel; generates its read-record arrays in HBM and loads them."""
        mc = model.as_c()
        _lib.check(self._lib.lsg_synth_reads(self._h, C.byref(mc)), "lsg_synth_reads")

    def synth_generate(self, model) -> Reads:
        """Only generates the model's compact read-record arrays in HBM (owned by the handle until the next generate / synth_reads)
        and returns their lsg_reads: a stand-in for a caller with a device-resident decoded BAM (bench.py times load_reads on it)."""
        mc = model.as_c()
        out = Reads()
        _lib.check(self._lib.lsg_synth_generate(self._h, C.byref(mc), C.byref(out)), "lsg_synth_generate")
        return out

    def reads_shape(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.lsg_get_reads_shape(self._h, C.byref(a), C.byref(b), C.byref(c)), "lsg_get_reads_shape")
        return int(a.value), int(b.value), int(c.value)

    def reads_to_host(self, events: bool = True) -> ReadRecords:
        """Copy the resident read-record arrays back to the host (tests, CPU-baseline sampling); the events need keep_reads.
        events=False: the per-read and per-segment arrays only (always resident; events and seg_ev_off come back empty / zero)."""
        R, S, E = self.reads_shape()
        arrs = {n: np.zeros({"read": R, "seg_": S, "even": E if events else 0}[n[:4]], dt) for n, dt in ReadRecords._SPEC}
        ptrs = [(_ptr(arrs[n]) if events or n not in ("events", "seg_ev_off") else None) for n, _ in ReadRecords._SPEC]
        r = Reads(R, S, E, *ptrs, 0)
        _lib.check(self._lib.lsg_copy_reads_to_host(self._h, C.byref(r)), "lsg_copy_reads_to_host")
        return ReadRecords(**arrs)

    def reference_to_host(self, tid: int) -> np.ndarray:
        out = np.zeros(int(self.contig_len[tid]), np.uint8)
        if out.size:
            _lib.check(self._lib.lsg_copy_reference_to_host(self._h, int(tid), _ptr(out)), "lsg_copy_reference_to_host")
        return out

    # ---- hot path ----------------------------------------------------------------------------
    def pileup_count(self, params: Optional[CountParams] = None):
        """Returns (rows per cell type, pileup columns with >= 1 counted entry summed over cell types)."""
        params = params or CountParams.longsom_defaults()
        n_rows = (C.c_int64 * _lib.MAX_CELLTYPES)()
        n_cols = C.c_int64(0)
        _lib.check(self._lib.lsg_pileup_count(self._h, C.byref(params), n_rows, C.byref(n_cols)), "lsg_pileup_count")
        self._n_rows = [int(n_rows[i]) for i in range(self.n_ct)]
        return list(self._n_rows), int(n_cols.value)

    def fetch_counts(self, ct: int):
        """Rows of one cell type in genomic order: keys int64 (tid<<32|pos0), ref uint8, counts uint32 [n,42]."""
        n = self._n_rows[ct]
        keys = np.empty(n, np.int64); ref = np.empty(n, np.uint8); counts = np.empty((n, ROW_WORDS), np.uint32)
        if n:
            _lib.check(self._lib.lsg_fetch_counts(self._h, ct, _ptr(keys), _ptr(ref), _ptr(counts), n), "lsg_fetch_counts")
        return keys, ref, counts

    def load_counts(self, keys_per_ct, counts_per_ct):
        """Install per-cell-type count rows (parsed from BaseCellCounter TSVs) instead of running the pileup."""
        n_ct = len(keys_per_ct)
        ks = [np.ascontiguousarray(k, dtype=np.int64) for k in keys_per_ct]
        cs = [np.ascontiguousarray(c, dtype=np.uint32).reshape(-1, ROW_WORDS) for c in counts_per_ct]
        kp = (C.c_void_p * n_ct)(*[k.ctypes.data for k in ks])
        cp = (C.c_void_p * n_ct)(*[c.ctypes.data for c in cs])
        nr = (C.c_int64 * n_ct)(*[len(k) for k in ks])
        _lib.check(self._lib.lsg_load_counts(self._h, n_ct, kp, cp, nr), "lsg_load_counts")
        self.n_ct = n_ct
        self._n_rows = [len(k) for k in ks]

    def max_live_reads(self) -> int:
        """Upper bound on the reads simultaneously live in the reference's pileup buffer (see lsg_max_live_reads)."""
        v = int(self._lib.lsg_max_live_reads(self._h))
        _lib.check(-1 if v < 0 else 0, "lsg_max_live_reads")
        return v

    def count_stats(self) -> CountStats:
        s = CountStats()
        _lib.check(self._lib.lsg_get_count_stats(self._h, C.byref(s)), "lsg_get_count_stats")
        return s

    def layout_info(self):
        """(path, build_ms, store_bytes): path 2 = the load built the store alone, 3 = in the pass that also made the first count (set_count_at_load), 4 = the load counted and kept no store (set_store_policy),
        5 = the same over tile-phased events (every entry fetched as its one 128-byte line), 6 = the same with the entries binned by
        128-position windows (one 256-byte block per entry); wall time the last load spent building the store; device bytes the store and what belongs to it hold (lsg_get_layout_info)"""
        path = C.c_int32(0); ms = C.c_double(0.0); nbytes = C.c_int64(0)
        _lib.check(self._lib.lsg_get_layout_info(self._h, C.byref(path), C.byref(ms), C.byref(nbytes)), "lsg_get_layout_info")
        return int(path.value), float(ms.value), int(nbytes.value)

    def build_times(self):
        """HIP-event ms of the last load's build: capacities + scatter, sort, per-entry words, event gather (lsg_get_build_times)"""
        ms = (C.c_float * 4)()
        _lib.check(self._lib.lsg_get_build_times(self._h, ms), "lsg_get_build_times")
        return [float(x) for x in ms]

    def store_shape(self):
        """(entries, 1 KB blocks, events) of the resident tile store (lsg_get_store_shape)"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.lsg_get_store_shape(self._h, C.byref(a), C.byref(b), C.byref(c)), "lsg_get_store_shape")
        return int(a.value), int(b.value), int(c.value)

    def max_live_reads_all(self) -> int:
        """the bound of max_live_reads over every resident read with a barcode, whatever its cell type (lsg_max_live_reads_all)"""
        v = int(self._lib.lsg_max_live_reads_all(self._h))
        _lib.check(-1 if v < 0 else 0, "lsg_max_live_reads_all")
        return v

    def max_live_reads_exact(self) -> int:
        """per cell type, per POSITION: the largest buffer a pushed read can meet, itself included - a count with max_depth >= this
        drops nothing (lsg_max_live_reads_exact)"""
        v = int(self._lib.lsg_max_live_reads_exact(self._h))
        _lib.check(-1 if v < 0 else 0, "lsg_max_live_reads_exact")
        return v

    def call_step1(self, params: Optional[CallParams] = None):
        params = params or CallParams.longsom_defaults()
        n_sites = C.c_int64(0); n_cand = C.c_int64(0)
        _lib.check(self._lib.lsg_call_step1(self._h, C.byref(params), C.byref(n_sites), C.byref(n_cand)), "lsg_call_step1")
        self._n_sites = int(n_sites.value); self._n_cand = int(n_cand.value)
        return self._n_sites, self._n_cand

    def fetch_calls(self, candidates_only: bool = False):
        cap = self._n_sites
        arr = np.empty(max(cap, 1), np.dtype(_lib.Call))
        n_out = C.c_int64(0)
        _lib.check(self._lib.lsg_fetch_calls(self._h, C.c_void_p(arr.ctypes.data), cap, 1 if candidates_only else 0, C.byref(n_out)), "lsg_fetch_calls")
        return arr[:int(n_out.value)]

    def export_calls(self, kind: int, dst_device_ptr: int = 0, capacity: int = 0) -> int:
        """Compact call records into a caller-owned device buffer (kind: 0 all, 1 step-2 rows, 2 PASS
        candidates); dst 0 = count only.  Returns the number of selected rows."""
        n_out = C.c_int64(0)
        _lib.check(self._lib.lsg_export_calls(self._h, int(kind), C.c_void_p(int(dst_device_ptr)) if dst_device_ptr else None,
                                              int(capacity), C.byref(n_out)), "lsg_export_calls")
        return int(n_out.value)

    # ---- the tables' text, printed on the device (include/longsom_hip.h: enum lsg_table) ----
    TABLE_COUNTS, TABLE_MERGED, TABLE_STEP1, TABLE_STEP1_KEPT, TABLE_STEP2, TABLE_STEP3_ROWS = 0, 4, 5, 6, 7, 8
    TABLE_CELL_LONG, TABLE_CELL_DP, TABLE_CELL_ALT, TABLE_CELL_VAF, TABLE_CELL_BIN = 9, 10, 11, 12, 13
    TABLE_BNPC_BIN, TABLE_BNPC_VAF = 14, 15
    TABLE_FASTQ = 16

    def bam_fastq(self, path: str, barcodes=None, celltype_of=None, n_celltypes: int = 0, min_mapq: int = 60, first_record_offset: Optional[int] = None) -> dict:
        """lsg_bam_fastq: the BAM's records as the FASTQ text ctat-LR-fusion reads (BamToFastq.py:9-42), printed on the device into table
        TABLE_FASTQ - fetch it with table_bytes(TABLE_FASTQ, sum(info["n_bytes"])) or stream it into a file with append_table.  barcodes
        None: plain mode, every record in file order.  barcodes (cleaned strings) + celltype_of + n_celltypes: routed mode, the records
        SplitBamCellTypes would write to a cell type's BAM (under min_mapq and set_split_filters' limits), cell type after cell type
        (FusionCalling.smk:3-37).  Reads and changes nothing of a resident load.  Returns the info dict (n_records, n_printed, n_bytes,
        bad_ordinal, bad_kind, the phases' times).  Raises _lib.LsgError for a record that cannot be printed (the error names it; .info
        holds bad_ordinal / bad_kind) and, with "straddle" in its text (rc -4), for a BAM to print on the host (hostio.bam_fastq)."""
        import mmap
        from . import hostio
        from ._lib import FastqInfo
        if first_record_offset is None:
            first_record_offset = hostio.bam_header(path)[2]
        info = FastqInfo()
        joined, n_cb, ct = None, 0, None
        if barcodes is not None:
            joined, n_cb = "\n".join(barcodes).encode(), len(barcodes)
            ct = np.ascontiguousarray(celltype_of, np.int32)
            if len(ct) != n_cb:
                raise ValueError("celltype_of holds %d entries for %d barcodes" % (len(ct), n_cb))
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                buf = np.frombuffer(mm, dtype=np.uint8)
                try:
                    rc = self._lib.lsg_bam_fastq(self._h, C.c_void_p(buf.ctypes.data), size, int(first_record_offset), joined, n_cb, _ptr(ct), int(n_celltypes),
                                                 int(min_mapq), C.byref(info))
                finally:
                    del buf
        d = hostio.fastq_info_dict(info)
        try:
            _lib.check(rc, "lsg_bam_fastq")
        except _lib.LsgError as e:
            e.info = d
            raise
        return d

    TABLE_SPLIT_BAM, TABLE_BGZF = 23, 27       # TABLE_SPLIT_BAM + t: cell type t's BAM file (t < 4); the file of bgzf_compress's bytes

    def split_bam(self, path: str, barcodes, celltype_of, n_celltypes: int, min_mapq: int = 60, first_record_offset: Optional[int] = None) -> dict:
        """lsg_split_bam: SplitBamCellTypes on the device (SplitBamCellTypes.py:39-192) - the BAM's records routed by cleaned CB to one BAM
        file per cell type under min_mapq and set_split_filters' limits (--n_trim honoured: the window's qualities are written as 0), cut
        into BGZF blocks as htslib cuts them, deflated on the device.  The files are tables TABLE_SPLIT_BAM + t: fetch them with
        table_bytes(TABLE_SPLIT_BAM + t, info["n_file_bytes"][t]) or stream them into files with append_table.  Reads and changes nothing
        of a resident load.  Returns the info dict (counters, reasons_n, reasons_first - hostio.split_report's inputs -, n_written,
        n_ubytes, n_blocks, n_file_bytes, bad_ordinal, bad_kind, the phases' times).  Raises _lib.LsgError (.info holds the dict) for a
        read the reference raises on, with rc -4 for a BAM to split on the host (hostio.split_bam) and rc -3 for one that does not fit."""
        import mmap
        from . import hostio
        from ._lib import SplitInfo
        if first_record_offset is None:
            first_record_offset = hostio.bam_header(path)[2]
        info = SplitInfo()
        joined, n_cb = "\n".join(barcodes).encode(), len(barcodes)
        ct = np.ascontiguousarray(celltype_of, np.int32)
        if len(ct) != n_cb:
            raise ValueError("celltype_of holds %d entries for %d barcodes" % (len(ct), n_cb))
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                buf = np.frombuffer(mm, dtype=np.uint8)
                try:
                    rc = self._lib.lsg_split_bam(self._h, C.c_void_p(buf.ctypes.data), size, int(first_record_offset), joined, n_cb, _ptr(ct), int(n_celltypes),
                                                 int(min_mapq), C.byref(info))
                finally:
                    del buf
        d = {k: getattr(info, k) for k, _ in info._fields_}
        for k in ("counters", "reasons_n", "reasons_first", "n_written", "n_ubytes", "n_blocks", "n_file_bytes"):
            d[k] = [int(x) for x in d[k]]
        failed = None
        try:                                            # (the call's own error text, read before anything else is asked of the library)
            _lib.check(rc, "lsg_split_bam")
        except _lib.LsgError as e:
            failed = e
        if self._split_index:                           # set_split_index: the cell types' indexes the call made (up to the one it refused)
            d["index"] = []
            for t in range(int(n_celltypes)):
                bi = _lib.BaiInfo()
                if self._lib.lsg_get_split_index_info(self._h, t, C.byref(bi)) != 0:
                    break
                d["index"].append({k: getattr(bi, k) for k, _ in bi._fields_ if k != "pad_"})
        if failed is not None:
            failed.info = d
            raise failed
        return d

    TABLE_SPLIT_BAI, TABLE_BAI = 28, 32        # TABLE_SPLIT_BAI + t: the .bai of cell type t's BAM (set_split_index); bam_index's .bai
    _split_index = False

    def set_split_index(self, on: bool) -> None:
        """lsg_set_split_index: split_bam also makes the .bai of every cell type's BAM (tables TABLE_SPLIT_BAI + t, their infos as
        info["index"][t]; fetch with table_bytes(TABLE_SPLIT_BAI + t, info["index"][t]["n_bytes"])) out of the routing's own arrays.  An
        input that is not coordinate-sorted then fails the call.  Off by default: split_bam is what it was."""
        _lib.check(self._lib.lsg_set_split_index(self._h, 1 if on else 0), "lsg_set_split_index")
        self._split_index = bool(on)

    def bam_index(self, path: str, first_record_offset: Optional[int] = None) -> dict:
        """lsg_bam_index: the .bai of a coordinate-sorted BAM - bins, chunks, the linear index, n_no_coor: samtools index / pysam.index in
        this project's canonical form (the host twin is hostio.build_bai(full=True)) - made on the device into table
        TABLE_BAI: fetch it with table_bytes(TABLE_BAI, info["n_bytes"]) or stream it into a file with append_table.  Returns the info dict.
        Raises _lib.LsgError (.info holds the dict: bad_ordinal / bad_kind = hostio.BAI_ERR_*) for a file that is not sorted, a negative
        position or an end beyond 2^29; with rc -4 / -3 for a BAM to index on the host."""
        import mmap
        from . import hostio
        if first_record_offset is None:
            first_record_offset = hostio.bam_header(path)[2]
        info = _lib.BaiInfo()
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                buf = np.frombuffer(mm, dtype=np.uint8)
                try:
                    rc = self._lib.lsg_bam_index(self._h, C.c_void_p(buf.ctypes.data), size, int(first_record_offset), C.byref(info))
                finally:
                    del buf
        d = {k: getattr(info, k) for k, _ in info._fields_ if k != "pad_"}
        try:
            _lib.check(rc, "lsg_bam_index")
        except _lib.LsgError as e:
            e.info = d
            raise
        return d

    def bgzf_compress(self, data) -> bytes:
        """lsg_bgzf_compress: the bytes as one BGZF file (blocks of 0xff00 bytes deflated on the device, the EOF block) - what gzip,
        htslib and load_bam read"""
        data = bytes(data)
        n = C.c_int64(0)
        buf = np.frombuffer(data, dtype=np.uint8)
        _lib.check(self._lib.lsg_bgzf_compress(self._h, C.c_void_p(buf.ctypes.data) if len(data) else None, len(data), C.byref(n)), "lsg_bgzf_compress")
        out = self.table_bytes(self.TABLE_BGZF, int(n.value))
        self.free_table(self.TABLE_BGZF)
        return out

    def set_table_names(self, contig_names, celltype_names) -> None:
        """Names the rows print (contigs in set_contigs order, cell types in index order)."""
        _lib.check(self._lib.lsg_set_table_names(self._h, len(contig_names), "\n".join(contig_names).encode(), len(celltype_names),
                                                 "\n".join(celltype_names).encode()), "lsg_set_table_names")

    def format_table(self, table: int) -> int:
        """Prints the rows of one table (TABLE_COUNTS + cell type, TABLE_MERGED, TABLE_STEP1, TABLE_STEP1_KEPT) into a device buffer the
        engine keeps; returns the size of the text."""
        n = C.c_int64(0)
        _lib.check(self._lib.lsg_format_table(self._h, int(table), C.byref(n)), "lsg_format_table")
        return int(n.value)

    def table_bytes(self, table: int, n_bytes: int, prefix: bytes = b"") -> bytes:
        """prefix + the formatted text as one bytes object."""
        api = C.pythonapi
        api.PyBytes_FromStringAndSize.restype = C.py_object
        api.PyBytes_FromStringAndSize.argtypes = [C.c_void_p, C.c_ssize_t]
        api.PyBytes_AsString.restype = C.c_void_p
        api.PyBytes_AsString.argtypes = [C.py_object]
        out = api.PyBytes_FromStringAndSize(None, len(prefix) + n_bytes)      # (uninitialised: filled below before anybody else sees it)
        at = api.PyBytes_AsString(out)
        if prefix:
            C.memmove(at, prefix, len(prefix))
        _lib.check(self._lib.lsg_copy_table(self._h, int(table), C.c_void_p(at + len(prefix)), n_bytes), "lsg_copy_table")
        return out

    def append_table(self, table: int, path: str) -> None:
        """Appends the formatted text to `path`; may run on a thread of its own beside other calls (not beside format_table / free_table
        of the same table)."""
        import os
        _lib.check(self._lib.lsg_append_table(self._h, int(table), os.fsencode(path)), "lsg_append_table")

    def step2_summary(self, n_cols: int):
        """After format_table(TABLE_STEP2): (kinds of cell per column over all its rows - the bits of tsvio.column_kinds -, size of the rows
        step 3 can keep, which are table TABLE_STEP3_ROWS now)."""
        kinds = np.zeros(int(n_cols), np.uint8)
        n = C.c_int64(0)
        _lib.check(self._lib.lsg_step2_summary(self._h, int(n_cols), _ptr(kinds), C.byref(n)), "lsg_step2_summary")
        return kinds, int(n.value)

    def free_table(self, table: int = -1) -> None:
        _lib.check(self._lib.lsg_free_table(self._h, int(table)), "lsg_free_table")

    # ---- the high-confidence cancer variant filter over a step-2 table's text (csrc/hccv.hip; reanno.hccv_filter_device drives it) ----
    TABLE_HCCV2, TABLE_HCCV3, TABLE_HCCV_PASS = 18, 19, 20

    def hccv_filter(self, params):
        """After format_table(TABLE_STEP2): its rows through HighConfidenceCancerVariants.py's row rules (an _lib.HccvParams) into
        TABLE_HCCV2 (.HCCV.tsv2's rows), TABLE_HCCV3 (.HCCV.tsv3's) and TABLE_HCCV_PASS (its PASS rows); returns the _lib.HccvInfo.
        info.n_undecided > 0: no table was made, the table is for reanno.hccv_filter."""
        info = _lib.HccvInfo()
        _lib.check(self._lib.lsg_hccv_filter(self._h, C.byref(params), C.byref(info)), "lsg_hccv_filter")
        return info

    def hccv_filter_text(self, text: bytes, params):
        """The same over a step-2 table in host memory (leading '#' lines skipped); info.kinds = the kinds of cell of its columns."""
        info = _lib.HccvInfo()
        _lib.check(self._lib.lsg_hccv_filter_text(self._h, text, len(text), C.byref(params), C.byref(info)), "lsg_hccv_filter_text")
        return info

    # ---- step 3's final filters over a step-2 table's text (csrc/step3.hip; calling.step3_device drives it) ----
    TABLE_STEP3_ALL, TABLE_STEP3_PASS = 21, 22

    def step3_filter(self, params):
        """After step2_summary: the rows of TABLE_STEP3_ROWS through BaseCellCalling.step3.py's row rules and its cluster test (an
        _lib.Step3Params) into TABLE_STEP3_ALL (calling.step3.unfiltered.tsv's rows) and TABLE_STEP3_PASS (calling.step3.tsv's); returns
        the _lib.Step3Info.  info.n_undecided > 0: no table was made, the rows are for calling.step3."""
        info = _lib.Step3Info()
        _lib.check(self._lib.lsg_step3_filter(self._h, C.byref(params), C.byref(info)), "lsg_step3_filter")
        return info

    def step3_filter_text(self, text: bytes, params):
        """The same over a whole step-2 table in host memory (leading '#' lines skipped); info.kinds = the kinds of cell of its columns."""
        info = _lib.Step3Info()
        _lib.check(self._lib.lsg_step3_filter_text(self._h, text, len(text), C.byref(params), C.byref(info)), "lsg_step3_filter_text")
        return info

    def load_posset(self, kind: int, keys, on_device: bool = False, n: Optional[int] = None):
        if on_device:
            _lib.check(self._lib.lsg_load_posset(self._h, kind, C.c_void_p(int(keys)), int(n), 1), "lsg_load_posset")
            return
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        _lib.check(self._lib.lsg_load_posset(self._h, kind, _ptr(keys), len(keys), 0), "lsg_load_posset")

    def load_alleleset(self, keys, on_device: bool = False, n: Optional[int] = None) -> None:
        """Step 2's gnomAD alleles (calling.pack_allele_keys, sorted and unique) resident for format_table(TABLE_STEP2); an empty array is
        a source that hits nothing, keys=None unloads the set (the table is then step 2's without a gnomAD source)."""
        if keys is None:
            _lib.check(self._lib.lsg_load_alleleset(self._h, None, -1, 0), "lsg_load_alleleset")
            return
        if on_device:
            _lib.check(self._lib.lsg_load_alleleset(self._h, C.c_void_p(int(keys)), int(n), 1), "lsg_load_alleleset")
            return
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        _lib.check(self._lib.lsg_load_alleleset(self._h, _ptr(keys), len(keys), 0), "lsg_load_alleleset")

    def probe_alleleset(self, keys) -> np.ndarray:
        """membership (uint8) of allele keys in the loaded set"""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        hits = np.zeros(len(keys), np.uint8)
        _lib.check(self._lib.lsg_probe_alleleset(self._h, _ptr(keys), len(keys), _ptr(hits), 0), "lsg_probe_alleleset")
        return hits

    def step2_allele_queries(self) -> np.ndarray:
        """After call_step1 and set_table_names: the allele keys of the rows step 2 keeps whose ALT is one base, in TABLE_STEP1_KEPT's row
        order (counted, then compacted, on the device)."""
        n = C.c_int64(0)
        _lib.check(self._lib.lsg_step2_allele_queries(self._h, None, 0, C.byref(n)), "lsg_step2_allele_queries")
        keys = np.zeros(int(n.value), np.int64)
        if len(keys):
            _lib.check(self._lib.lsg_step2_allele_queries(self._h, _ptr(keys), len(keys), C.byref(n)), "lsg_step2_allele_queries")
        return keys

    def genotype_cells(self, site_keys, alt_sym, params=None):
        """Per-cell (Dp, Alt) at target sites (HCCVSingleCellGenotype.py:82-220).  site_keys = (tid << 32) | pos0, strictly
        ascending; alt_sym = expected alt symbol class per site.  Returns two uint32 arrays [n_sites, n_cb]."""
        from ._lib import GenotypeParams
        params = params or GenotypeParams.longsom_defaults()
        site_keys = np.ascontiguousarray(site_keys, dtype=np.int64)
        alt_sym = np.ascontiguousarray(alt_sym, dtype=np.uint8)
        assert len(site_keys) == len(alt_sym)
        dp = np.zeros((len(site_keys), self.n_cb), np.uint32)
        alt = np.zeros((len(site_keys), self.n_cb), np.uint32)
        if len(site_keys):
            _lib.check(self._lib.lsg_genotype_cells(self._h, C.byref(params), len(site_keys), _ptr(site_keys), _ptr(alt_sym), _ptr(dp), _ptr(alt), 0),
                       "lsg_genotype_cells")
        return dp, alt

    def genotype_cells_grouped(self, site_keys, alt_sym, group_off, params=None, max_depth: int = 200000):
        """genotype_cells with the pileup's depth cap replayed per window of target sites (lsg_genotype_cells_grouped): the sites
        [group_off[g], group_off[g + 1]) are one pileup call of the reference (HCCVSingleCellGenotype.py:109-122)."""
        from ._lib import GenotypeParams
        params = params or GenotypeParams.longsom_defaults()
        site_keys = np.ascontiguousarray(site_keys, dtype=np.int64)
        alt_sym = np.ascontiguousarray(alt_sym, dtype=np.uint8)
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        assert len(site_keys) == len(alt_sym)
        dp = np.zeros((len(site_keys), self.n_cb), np.uint32)
        alt = np.zeros((len(site_keys), self.n_cb), np.uint32)
        if len(site_keys):
            _lib.check(self._lib.lsg_genotype_cells_grouped(self._h, C.byref(params), int(max_depth), len(site_keys), _ptr(site_keys), _ptr(alt_sym),
                                                            len(group_off) - 1, _ptr(group_off), _ptr(dp), _ptr(alt), 0), "lsg_genotype_cells_grouped")
        return dp, alt

    # ---- per-cell verdicts and cell-by-variant matrices (CellClustering/SingleCellGenotype.py; csrc/cellgeno.hip) ----
    CELL_NOCOVERAGE, CELL_NOALT, CELL_LOWVAF_CHRM, CELL_BETABIN_PROBLEM, CELL_PASS = 0, 1, 2, 3, 4
    CELL_STATUS_NAMES = ["NoCoverage", "NoAltReads", "LowVAFChrM", "BetaBin_problem", "PASS"]

    def cellgeno_count(self, site_keys, alt_sym, is_chrm, group_off, params=None, max_depth: int = 200000, alpha2: float = 0.2474528917555431,
                       beta2: float = 162.03696139428595, pvalue: float = 0.01) -> None:
        """genotype_cells_grouped + the verdict of every (site, barcode) cell (SingleCellGenotype.py:181-218), all left on the device:
        cellgeno_fetch copies them out, cellgeno_set_text + format_table(TABLE_CELL_*) print them.  is_chrm: per site, 1 where the
        chrM rule applies (--chrM_contaminant True and a contig named chrM)."""
        from ._lib import GenotypeParams
        params = params or GenotypeParams.longsom_defaults(strict_cb=0)
        site_keys = np.ascontiguousarray(site_keys, dtype=np.int64)
        alt_sym = np.ascontiguousarray(alt_sym, dtype=np.uint8)
        is_chrm = np.ascontiguousarray(is_chrm, dtype=np.uint8)
        group_off = np.ascontiguousarray(group_off, dtype=np.int64)
        assert len(site_keys) == len(alt_sym) == len(is_chrm)
        _lib.check(self._lib.lsg_cellgeno_count(self._h, C.byref(params), int(max_depth), len(site_keys), _ptr(site_keys), _ptr(alt_sym), _ptr(is_chrm),
                                                max(len(group_off) - 1, 0), _ptr(group_off), float(alpha2), float(beta2), float(pvalue)), "lsg_cellgeno_count")
        self._cell_shape = (len(site_keys), self.n_cb); self._cells_only = False; self._filter_shape = self._mat_shape = None

    def cellgeno_load_counts(self, dp, alt, is_chrm, alpha2: float = 0.2474528917555431, beta2: float = 162.03696139428595, pvalue: float = 0.01) -> None:
        """The same verdicts for Dp / Alt tables [n_sites, n_cb] the caller brings instead of a count."""
        dp = np.ascontiguousarray(dp, dtype=np.uint32); alt = np.ascontiguousarray(alt, dtype=np.uint32)
        is_chrm = np.ascontiguousarray(is_chrm, dtype=np.uint8)
        assert dp.ndim == 2 and dp.shape == alt.shape and len(is_chrm) == dp.shape[0]
        _lib.check(self._lib.lsg_cellgeno_load_counts(self._h, dp.shape[0], dp.shape[1], _ptr(dp), _ptr(alt), _ptr(is_chrm), float(alpha2), float(beta2), float(pvalue)),
                   "lsg_cellgeno_load_counts")
        self._cell_shape = dp.shape; self._cells_only = False; self._filter_shape = self._mat_shape = None

    def cellgeno_load_cells(self, bin, vaf4) -> None:
        """bin [n_sites, n_cb] in {0, 1, 3} and vaf4 (VAF * 1e4, -1 for NA) parsed from matrix files, made resident as the verdicts of a
        count would be (lsg_cellgeno_load_cells): for cellgeno_set_text + cellgeno_filter.  There are no counts behind them: the long
        table, the Dp / Alt matrices and dp / alt / p4 of cellgeno_fetch are refused."""
        bin = np.ascontiguousarray(bin, dtype=np.uint8); vaf4 = np.ascontiguousarray(vaf4, dtype=np.int32)
        assert bin.ndim == 2 and bin.shape == vaf4.shape
        _lib.check(self._lib.lsg_cellgeno_load_cells(self._h, bin.shape[0], bin.shape[1], _ptr(bin), _ptr(vaf4)), "lsg_cellgeno_load_cells")
        self._cell_shape = bin.shape; self._cells_only = True; self._filter_shape = self._mat_shape = None

    def cellgeno_filter(self, min_cells_per_mut: int, min_pos_cov: int, col_int_ok):
        """FormatInputBnpC.py's two filters over the rows of mat_order and the columns of col_src (lsg_cellgeno_filter); col_int_ok: per
        column, whether nothing on the host's side makes it a float column.  Returns (rows kept, columns kept);
        format_table(TABLE_BNPC_BIN / TABLE_BNPC_VAF) print them."""
        ok = np.ascontiguousarray(col_int_ok, dtype=np.uint8)
        shape = getattr(self, "_mat_shape", None)
        if shape is not None and len(ok) != shape[1]:                                   # (the library reads one flag per column of col_src)
            raise ValueError("cellgeno_filter: %d flags for %d columns" % (len(ok), shape[1]))
        n_rows, n_cols = C.c_int64(0), C.c_int32(0)
        _lib.check(self._lib.lsg_cellgeno_filter(self._h, int(min_cells_per_mut), int(min_pos_cov), _ptr(ok), C.byref(n_rows), C.byref(n_cols)), "lsg_cellgeno_filter")
        self._filter_shape = (self._mat_shape[0], len(ok))
        return int(n_rows.value), int(n_cols.value)

    def cellgeno_filter_fetch(self) -> dict:
        """row_keep, row_mut per row of mat_order; col_keep, col_cov_kept, col_cov_all, col_int per column, of the last cellgeno_filter"""
        shape = getattr(self, "_filter_shape", None)
        if shape is None:
            raise _lib.LsgError("cellgeno_filter_fetch: nothing filtered (cellgeno_filter first)")
        out = dict(row_keep=np.zeros(shape[0], np.uint8), col_keep=np.zeros(shape[1], np.uint8), row_mut=np.zeros(shape[0], np.int32),
                   col_cov_kept=np.zeros(shape[1], np.int32), col_cov_all=np.zeros(shape[1], np.int32), col_int=np.zeros(shape[1], np.uint8))
        _lib.check(self._lib.lsg_cellgeno_filter_fetch(self._h, *[_ptr(out[k]) for k in ("row_keep", "col_keep", "row_mut", "col_cov_kept", "col_cov_all", "col_int")]),
                   "lsg_cellgeno_filter_fetch")
        return out

    def cellgeno_fetch(self, cells: bool = True) -> dict:
        """dp, alt, vaf4, p4, status, bin [n_sites, n_cb] (cells=False: not these) and n_covered, n_pass [n_cb] of the last cellgeno_count /
        cellgeno_load_counts."""
        shape = getattr(self, "_cell_shape", None)
        if shape is None:
            raise _lib.LsgError("cellgeno_fetch: nothing classified (cellgeno_count first)")
        out = {"n_covered": np.zeros(shape[1], np.int64), "n_pass": np.zeros(shape[1], np.int64)}
        if cells:
            out.update(dp=np.zeros(shape, np.uint32), alt=np.zeros(shape, np.uint32), vaf4=np.zeros(shape, np.int32), p4=np.zeros(shape, np.int32),
                       status=np.zeros(shape, np.uint8), bin=np.zeros(shape, np.uint8))
            if getattr(self, "_cells_only", False):                                    # cellgeno_load_cells: no counts, no tails
                for k in ("dp", "alt", "p4"):
                    del out[k]
        _lib.check(self._lib.lsg_cellgeno_fetch(self._h, *[_ptr(out.get(k)) for k in ("dp", "alt", "vaf4", "p4", "status", "bin", "n_covered", "n_pass")]), "lsg_cellgeno_fetch")
        return out

    def cellgeno_set_text(self, heads, indexes, labels, barcodes, celltypes, long_order, mat_order, col_src, float_cells: bool) -> None:
        """The strings (per site: heads, indexes, labels; per barcode: barcodes, celltypes) and orders the tables TABLE_CELL_* print
        (include/longsom_hip.h: lsg_cellgeno_text)."""
        from ._lib import CellGenoText

        def blob(strings):
            enc = [s.encode() for s in strings]
            off = np.zeros(len(enc) + 1, np.uint32)
            if enc:
                off[1:] = np.cumsum([len(e) for e in enc])
            return b"".join(enc), off
        parts = [blob(x) for x in (heads, indexes, labels, barcodes, celltypes)]
        lo = np.ascontiguousarray(long_order, dtype=np.int32); mo = np.ascontiguousarray(mat_order, dtype=np.int32); cs = np.ascontiguousarray(col_src, dtype=np.int32)
        t = CellGenoText()
        for name, (b, off) in zip(("head", "index", "label", "cb", "ct"), parts):
            setattr(t, name, b); setattr(t, name + "_off", off.ctypes.data)
        t.n_long, t.long_order, t.n_mat, t.mat_order = len(lo), lo.ctypes.data, len(mo), mo.ctypes.data
        t.n_cols, t.float_cells, t.col_src = len(cs), 1 if float_cells else 0, cs.ctypes.data
        self._filter_shape = self._mat_shape = None
        _lib.check(self._lib.lsg_cellgeno_set_text(self._h, C.byref(t)), "lsg_cellgeno_set_text")
        self._mat_shape = (len(mo), len(cs))

    # ---- cell-by-gene read counts (rules/CNACalling.smk:11-75; csrc/genecounts.hip; longsom_amd/genecounts.py states the contract) ----
    TABLE_GENE_COUNTS = 17

    def load_annotation(self, ann, row_of_gene, n_rows: int) -> None:
        """The flattened exons (a genecounts.Annotation) and the matrix row every gene adds to (-1: assigned, printed nowhere) resident
        for gene_counts (lsg_load_annotation).  Drops a matrix counted under another annotation."""
        keys = np.ascontiguousarray(ann.keys, dtype=np.uint64); lens = np.ascontiguousarray(ann.lens, dtype=np.uint32)
        labels = np.ascontiguousarray(ann.labels, dtype=np.uint32); rows = np.ascontiguousarray(row_of_gene, dtype=np.int32)
        if not (len(keys) == len(lens) == len(labels)) or len(rows) != ann.n_genes:
            raise ValueError("load_annotation: %d keys, %d lengths, %d labels; %d rows for %d genes" % (len(keys), len(lens), len(labels), len(rows), ann.n_genes))
        self._gene_shape = None
        _lib.check(self._lib.lsg_load_annotation(self._h, len(keys), _ptr(keys), _ptr(lens), _ptr(labels), len(rows), _ptr(rows), int(n_rows)), "lsg_load_annotation")
        self._gene_rows = int(n_rows)

    def gene_counts(self, min_mapq: int = 0, flag_exclude: int = 0x4) -> dict:
        """Counts the resident load's reads per (gene row, barcode) and ADDS them to the resident matrix and tallies (lsg_gene_counts):
        another load of the same sample accumulates.  Returns the call's info (its reads per outcome, the phases' times)."""
        from ._lib import GeneCountInfo, GeneCountParams
        p = GeneCountParams(int(min_mapq), int(flag_exclude)); info = GeneCountInfo()
        _lib.check(self._lib.lsg_gene_counts(self._h, C.byref(p), C.byref(info)), "lsg_gene_counts")
        self._gene_shape = (getattr(self, "_gene_rows", 0), self.n_cb)
        return {k: getattr(info, k) for k, _ in GeneCountInfo._fields_ if k != "pad_"}

    def gene_counts_fetch(self, matrix: bool = True):
        """(matrix uint32 [n_rows, n_cb] in barcode-id order or None, tallies uint64 [n_cb, 4]: Assigned, NoFeatures, Ambiguity, Filtered)"""
        shape = getattr(self, "_gene_shape", None)
        if shape is None:
            raise _lib.LsgError("gene_counts_fetch: nothing counted (gene_counts first)")
        m = np.zeros(shape, np.uint32) if matrix else None
        t = np.zeros((shape[1], 4), np.uint64)
        _lib.check(self._lib.lsg_gene_counts_fetch(self._h, _ptr(m), _ptr(t)), "lsg_gene_counts_fetch")
        return m, t

    def gene_counts_set_text(self, row_names, col_order, barcodes, sep: str = ",") -> None:
        """The strings format_table(TABLE_GENE_COUNTS) prints: the row names, the columns as barcode ids in output order (their strings
        are barcodes[id]) and the separator (lsg_gene_counts_set_text)."""
        def blob(strings):
            enc = [s.encode() for s in strings]
            off = np.zeros(len(enc) + 1, np.uint32)
            if enc:
                off[1:] = np.cumsum([len(e) for e in enc])
            return b"".join(enc), off
        order = np.ascontiguousarray(col_order, dtype=np.int32)
        rows, row_off = blob(row_names)
        cols, col_off = blob([barcodes[i] for i in order])
        if len(sep.encode()) != 1:
            raise ValueError("gene_counts_set_text: the separator is one byte")
        if len(row_names) != getattr(self, "_gene_rows", 0):                      # (the library reads one name per row of the annotation)
            raise ValueError("gene_counts_set_text: %d names for %d rows" % (len(row_names), getattr(self, "_gene_rows", 0)))
        _lib.check(self._lib.lsg_gene_counts_set_text(self._h, rows, row_off.ctypes.data, len(order), _ptr(order), cols, col_off.ctypes.data, ord(sep)), "lsg_gene_counts_set_text")

    def gene_counts_reset(self) -> None:
        """frees the annotation, the matrix, the tallies and the table's text (lsg_gene_counts_reset)"""
        _lib.check(self._lib.lsg_gene_counts_reset(self._h), "lsg_gene_counts_reset")
        self._gene_shape = None; self._gene_rows = 0

    # ---- BnpC's posterior estimate (CellClustering/libs/utils.py:90-245; csrc/bnpc.hip; longsom_amd/bnpc.py drives it) ----
    def bnpc_load_samples(self, assignments, params=None) -> None:
        """Posterior samples resident: assignments [S, N] (labels in [0, N)) and, for bnpc_mean_params, params [S, k_max, M] float32
        (lsg_bnpc_load_samples).  A second load replaces the first."""
        a = np.ascontiguousarray(assignments, dtype=np.int32)
        if a.ndim != 2:
            raise ValueError("bnpc_load_samples: assignments must be [samples, cells]")
        p = None
        if params is not None:
            p = np.ascontiguousarray(params, dtype=np.float32)
            if p.ndim != 3 or p.shape[0] != a.shape[0]:
                raise ValueError("bnpc_load_samples: params must be [samples, clusters, mutations] with one row block per sample")
        self._bnpc_shape = None
        _lib.check(self._lib.lsg_bnpc_load_samples(self._h, a.shape[0], a.shape[1], a.ctypes.data_as(C.c_void_p), p.shape[1] if p is not None else 0,
                                                   p.shape[2] if p is not None else 0, p.ctypes.data_as(C.c_void_p) if p is not None else None), "lsg_bnpc_load_samples")
        self._bnpc_shape = (a.shape[0], a.shape[1], p.shape[2] if p is not None else 0)

    def bnpc_codist(self, fetch: bool = True):
        """D[pair] = the samples in which the pair's labels differ, pdist's condensed order, uint32 (lsg_bnpc_codist); stays resident for bnpc_mpear"""
        _lib.check(self._lib.lsg_bnpc_codist(self._h), "lsg_bnpc_codist")
        if not fetch:
            return None
        n = self._bnpc_shape[1]
        out = np.zeros(n * (n - 1) // 2, np.uint32)
        _lib.check(self._lib.lsg_bnpc_fetch_dist(self._h, out.ctypes.data_as(C.c_void_p), len(out)), "lsg_bnpc_fetch_dist")
        return out

    def bnpc_mpear(self, cuts):
        """(same_pairs [n_cuts], same_sim [n_cuts], dist_sum) of candidate clusterings cuts [n_cuts, N] over the resident D (lsg_bnpc_mpear)"""
        cuts = np.ascontiguousarray(cuts, dtype=np.int32)
        shape = getattr(self, "_bnpc_shape", None)
        if shape is not None and (cuts.ndim != 2 or cuts.shape[1] != shape[1]):
            raise ValueError("bnpc_mpear: cuts must be [n_cuts, %d]" % shape[1])
        k = cuts.shape[0] if cuts.ndim == 2 else 0
        pairs = np.zeros(k, np.uint64); sim = np.zeros(k, np.uint64); dsum = C.c_uint64(0)
        _lib.check(self._lib.lsg_bnpc_mpear(self._h, k, _ptr(cuts), _ptr(pairs), _ptr(sim), C.byref(dsum)), "lsg_bnpc_mpear")
        return pairs, sim, int(dsum.value)

    def bnpc_mean_params(self, final_assign):
        """(params [C, M] float64, branch [C] uint8, n_used [C] int32) of a final assignment's clusters, its distinct values ascending (lsg_bnpc_mean_params)"""
        fa = np.ascontiguousarray(final_assign, dtype=np.int32)
        shape = getattr(self, "_bnpc_shape", None)
        if shape is not None and fa.shape != (shape[1],):
            raise ValueError("bnpc_mean_params: final_assign must be [%d]" % shape[1])
        n_cl = len(np.unique(fa))
        out = np.zeros((n_cl, shape[2] if shape else 0), np.float64); branch = np.zeros(n_cl, np.uint8); n_used = np.zeros(n_cl, np.int32)
        _lib.check(self._lib.lsg_bnpc_mean_params(self._h, fa.ctypes.data_as(C.c_void_p), n_cl, out.ctypes.data_as(C.c_void_p), _ptr(branch), _ptr(n_used)), "lsg_bnpc_mean_params")
        return out, branch, n_used

    def bnpc_linkage(self, fetch: bool = True):
        """scipy's linkage(D / S, "ward") of the resident D, Z [N - 1, 4] float64 (lsg_bnpc_linkage); the tree stays resident for bnpc_cut_tree"""
        shape = getattr(self, "_bnpc_shape", None)
        Z = np.zeros((shape[1] - 1, 4), np.float64) if fetch and shape is not None else None
        _lib.check(self._lib.lsg_bnpc_linkage(self._h, _ptr(Z) if Z is not None else None), "lsg_bnpc_linkage")
        return Z

    def bnpc_cut_tree(self, ns):
        """scipy's cut_tree(Z, n_clusters=ns) of the resident tree as rows: labels [len(ns), N] int32 (lsg_bnpc_cut_tree)"""
        ns = np.ascontiguousarray(np.atleast_1d(ns), dtype=np.int32)
        shape = getattr(self, "_bnpc_shape", None)
        labels = np.zeros((len(ns), shape[1] if shape is not None else 0), np.int32)
        _lib.check(self._lib.lsg_bnpc_cut_tree(self._h, len(ns), _ptr(ns), _ptr(labels)), "lsg_bnpc_cut_tree")
        return labels

    def bnpc_avg_cluster_number(self):
        """bnpc.avg_cluster_number of the resident samples: per sample the labels of more than 2 cells counted on the device
        (lsg_bnpc_cluster_counts), their integer sum divided once"""
        total = C.c_int64(0)
        _lib.check(self._lib.lsg_bnpc_cluster_counts(self._h, C.byref(total)), "lsg_bnpc_cluster_counts")
        return np.float64(total.value) / np.float64(self._bnpc_shape[0])

    def bnpc_unload(self) -> None:
        _lib.check(self._lib.lsg_bnpc_unload(self._h), "lsg_bnpc_unload")
        self._bnpc_shape = None

    # ---- BnpC's sampler (CellClustering/libs/CRP.py, libs/MCMC.py; csrc/bnpc_sampler.hip; longsom_amd/bnpc_sampler.py drives it) ----
    def bnpcs_create(self, model, seeds, steps: int, arena_rows: int) -> None:
        """The data of a bnpc_sampler.Model and the buffers of len(seeds) chains of `steps` steps resident (lsg_bnpcs_create)"""
        from scipy.special import betaln
        one, zero = model.masks64()
        cfg = np.array([model.FN, model.FP, model.p, model.q, model.g0, model.g1, model.dpa_prob,
                        np.log(model.mix[1] * (1 - model.FN) + model.mix[0] * model.FP), np.log(model.mix[1] * model.FN + model.mix[0] * (1 - model.FP)),
                        betaln(model.p, model.q)], np.float64)
        sd = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64)
        self._bnpcs_shape = None
        _lib.check(self._lib.lsg_bnpcs_create(self._h, model.N, model.M, len(sd), int(steps), _ptr(one), _ptr(zero), _ptr(cfg), _ptr(sd), int(arena_rows)), "lsg_bnpcs_create")
        self._bnpcs_shape = (len(sd), int(steps) + 1, model.N, model.M, int(arena_rows))

    def bnpcs_set_state(self, chain: int, labels, theta, alpha: float) -> None:
        """one chain's labels [N], theta [N, M] float32 (row = cluster id) and concentration (lsg_bnpcs_set_state)"""
        _, _, N, M, _ = self._bnpcs_shape
        lab = np.ascontiguousarray(labels, dtype=np.int32); th = np.ascontiguousarray(theta, dtype=np.float32)
        if lab.shape != (N,) or th.shape != (N, M):
            raise ValueError("bnpcs_set_state: labels must be [%d] and theta [%d, %d]" % (N, N, M))
        _lib.check(self._lib.lsg_bnpcs_set_state(self._h, int(chain), _ptr(lab), _ptr(th), float(alpha)), "lsg_bnpcs_set_state")

    def bnpcs_get_state(self, chain: int):
        """(labels [N] int32, theta [N, M] float32, alpha) of one chain (lsg_bnpcs_get_state)"""
        _, _, N, M, _ = self._bnpcs_shape
        lab = np.zeros(N, np.int32); th = np.zeros((N, M), np.float32); alpha = C.c_double(0)
        _lib.check(self._lib.lsg_bnpcs_get_state(self._h, int(chain), _ptr(lab), _ptr(th), C.byref(alpha)), "lsg_bnpcs_get_state")
        return lab, th, float(alpha.value)

    def bnpcs_run(self, first_step: int, n_steps: int, burn_in: int) -> int:
        """steps first_step .. first_step + n_steps - 1 of every chain; returns how many were recorded before the arena filled (lsg_bnpcs_run)"""
        done = C.c_int32(0)
        _lib.check(self._lib.lsg_bnpcs_run(self._h, int(first_step), int(n_steps), int(burn_in), C.byref(done)), "lsg_bnpcs_run")
        return int(done.value)

    def bnpcs_fetch(self):
        """(labels [C, steps + 1, N], scalars [C, steps + 1, 5], arena [C, arena_rows, M]) so far; empties the arena (lsg_bnpcs_fetch)"""
        Cn, S1, N, M, rows = self._bnpcs_shape
        labels = np.zeros((Cn, S1, N), np.int32); scalars = np.zeros((Cn, S1, 5), np.float64); arena = np.zeros((Cn, rows, M), np.float32)
        used = np.zeros(Cn, np.int64); self._bnpcs_errors = np.zeros(Cn, np.int32)
        _lib.check(self._lib.lsg_bnpcs_fetch(self._h, _ptr(labels), _ptr(scalars), _ptr(arena), _ptr(used), _ptr(self._bnpcs_errors)), "lsg_bnpcs_fetch")
        return labels, scalars, arena

    def bnpcs_set_split_merge(self, prob: float, ratio_split: float, ratio_merge: float, scans: int) -> None:
        """every chain takes the split-merge move with this probability per step (lsg_bnpcs_set_split_merge); after bnpcs_create"""
        _lib.check(self._lib.lsg_bnpcs_set_split_merge(self._h, float(prob), float(ratio_split), float(ratio_merge), int(scans)), "lsg_bnpcs_set_split_merge")

    def bnpcs_fetch_moves(self) -> np.ndarray:
        """[C, steps + 1] int8: 0 a sweep, 1 / 2 a split declined / accepted, 3 / 4 a merge declined / accepted (lsg_bnpcs_fetch_moves)"""
        Cn, S1, _, _, _ = self._bnpcs_shape
        moves = np.zeros((Cn, S1), np.int8)
        _lib.check(self._lib.lsg_bnpcs_fetch_moves(self._h, _ptr(moves)), "lsg_bnpcs_fetch_moves")
        return moves

    def bnpcs_set_error_learning(self, prob: float, fp_mean: float, fp_sd: float, fn_mean: float, fn_sd: float) -> None:
        """every chain gets error rates of its own, started at the priors' means, and updates them with this probability per step
        (lsg_bnpcs_set_error_learning); after bnpcs_create"""
        _lib.check(self._lib.lsg_bnpcs_set_error_learning(self._h, float(prob), float(fp_mean), float(fp_sd), float(fn_mean), float(fn_sd)), "lsg_bnpcs_set_error_learning")

    def bnpcs_set_error_rates(self, chain: int, fp: float, fn: float) -> None:
        """one chain's error rates (lsg_bnpcs_set_error_rates)"""
        _lib.check(self._lib.lsg_bnpcs_set_error_rates(self._h, int(chain), float(fp), float(fn)), "lsg_bnpcs_set_error_rates")

    def bnpcs_fetch_error_rates(self):
        """(rates [C, steps + 1, 2]: FP, FN as each step recorded them; counts [C, 4]: FP accepted, declined, FN accepted, declined)
        (lsg_bnpcs_fetch_error_rates)"""
        Cn, S1, _, _, _ = self._bnpcs_shape
        rates = np.zeros((Cn, S1, 2), np.float64); counts = np.zeros((Cn, 4), np.int32)
        _lib.check(self._lib.lsg_bnpcs_fetch_error_rates(self._h, _ptr(rates), _ptr(counts)), "lsg_bnpcs_fetch_error_rates")
        return rates, counts

    def bnpcs_set_fixed_assignment(self, on: bool) -> None:
        """the steps keep the loaded labels: no sweep, no split-merge move, no concentration update (lsg_bnpcs_set_fixed_assignment)"""
        _lib.check(self._lib.lsg_bnpcs_set_fixed_assignment(self._h, 1 if on else 0), "lsg_bnpcs_set_fixed_assignment")

    def bnpcs_errors(self) -> np.ndarray:
        """per chain, the gamma variates that ran out of tries, as of the last bnpcs_fetch"""
        return self._bnpcs_errors

    def bnpcs_extend(self, add_steps: int) -> None:
        """room for add_steps more recorded steps; the chains, their records, the arena and the next step stay (lsg_bnpcs_extend)"""
        _lib.check(self._lib.lsg_bnpcs_extend(self._h, int(add_steps)), "lsg_bnpcs_extend")
        Cn, S1, N, M, rows = self._bnpcs_shape
        self._bnpcs_shape = (Cn, S1 + int(add_steps), N, M, rows)

    def bnpcs_psrf(self, first, last: int) -> np.ndarray:
        """[C, 5] float64: n, the mean, the sample variance, tau(b), tau(b // 3) of every chain's ML records first[c] .. last - 1, computed
        on the device; nothing else comes to the host (lsg_bnpcs_psrf; bnpc_sampler.psrf_of_stats makes the PSRF of them)"""
        Cn = self._bnpcs_shape[0]
        fs = np.ascontiguousarray(first, dtype=np.int32)
        if fs.shape != (Cn,):
            raise ValueError("bnpcs_psrf: first must be [%d]" % Cn)
        stats = np.zeros((Cn, 5), np.float64)
        _lib.check(self._lib.lsg_bnpcs_psrf(self._h, _ptr(fs), int(last), _ptr(stats)), "lsg_bnpcs_psrf")
        return stats

    def bnpcs_test_set_ml(self, chain: int, first: int, values) -> None:
        """values as the chain's ML records first .. first + len(values) - 1 (lsg_bnpcs_test_set_ml)"""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        _lib.check(self._lib.lsg_bnpcs_test_set_ml(self._h, int(chain), int(first), len(v), _ptr(v)), "lsg_bnpcs_test_set_ml")

    def bnpcs_destroy(self) -> None:
        _lib.check(self._lib.lsg_bnpcs_destroy(self._h), "lsg_bnpcs_destroy")
        self._bnpcs_shape = None

    def bnpcs_test_stream(self, key: int, counters):
        ctr = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
        words = np.zeros_like(ctr); dbl = np.zeros((len(ctr), 2), np.float64)
        _lib.check(self._lib.lsg_bnpcs_test_stream(self._h, int(key), len(ctr), _ptr(ctr), _ptr(words), _ptr(dbl)), "lsg_bnpcs_test_stream")
        return words, dbl

    def bnpcs_test_variates(self, key: int, kind: int, n: int, a: float, b: float):
        out = np.zeros(n, np.float64); err = C.c_int32(0)
        _lib.check(self._lib.lsg_bnpcs_test_variates(self._h, int(key), int(kind), int(n), float(a), float(b), _ptr(out), C.byref(err)), "lsg_bnpcs_test_variates")
        return out, int(err.value)

    def bnpcs_test_counts(self, chain: int):
        _, _, N, M, _ = self._bnpcs_shape
        n1 = np.zeros((N, M), np.uint32); n0 = np.zeros((N, M), np.uint32)
        _lib.check(self._lib.lsg_bnpcs_test_counts(self._h, int(chain), _ptr(n1), _ptr(n0)), "lsg_bnpcs_test_counts")
        return n1, n0

    def bnpcs_test_ll(self, chain: int):
        _, _, N, M, _ = self._bnpcs_shape
        ll = np.zeros((N, N), np.float64); ids = np.zeros(N, np.int32); k = C.c_int32(0)
        _lib.check(self._lib.lsg_bnpcs_test_ll(self._h, int(chain), _ptr(ll), _ptr(ids), C.byref(k)), "lsg_bnpcs_test_ll")
        K = int(k.value)
        return ll.ravel()[:N * K].reshape(N, K).copy(), ids[:K].copy()

    def bnpcs_test_move(self, what: int, step: int) -> None:
        _lib.check(self._lib.lsg_bnpcs_test_move(self._h, int(what), int(step)), "lsg_bnpcs_test_move")

    def bnpcs_test_move_outcome(self, chain: int) -> dict:
        """a chain's last split-merge move (what = 2): code, clusters, anchors, A, terms [4], lv, n_S (lsg_bnpcs_test_move_outcome)"""
        o = np.zeros(12, np.float64)
        _lib.check(self._lib.lsg_bnpcs_test_move_outcome(self._h, int(chain), _ptr(o)), "lsg_bnpcs_test_move_outcome")
        return {"code": int(o[0]), "clusters": (int(o[1]), int(o[2])), "anchors": (int(o[3]), int(o[4])), "A": float(o[5]), "terms": o[6:10].copy(), "lv": float(o[10]),
                "n_S": int(o[11])}

    def bnpcs_test_error_outcome(self, chain: int):
        """a chain's last error-rate update (bnpcs_test_move(3, step)): None where its deciding draw said no update, else per rate a dict of
        pick (the sd's index), new, new_ll, old_ll, prior (new - old), new_p, old_p, A, lv and code (1 accepted, 0 declined, -1 declined
        because rounding put the proposal on an end) (lsg_bnpcs_test_error_outcome)"""
        o = np.zeros(21, np.float64)
        _lib.check(self._lib.lsg_bnpcs_test_error_outcome(self._h, int(chain), _ptr(o)), "lsg_bnpcs_test_error_outcome")
        if not o[0]:
            return None
        names = ("pick", "new", "new_ll", "old_ll", "prior", "new_p", "old_p", "A", "lv", "code")
        return {rate: {k: (int(v) if k in ("pick", "code") else float(v)) for k, v in zip(names, o[1 + 10 * e:11 + 10 * e])} for e, rate in enumerate(("FP", "FN"))}

    def betabinom_sf4(self, k, n, alpha: float, beta: float) -> np.ndarray:
        """round(betabinom.sf(k - 0.001, n, alpha, beta), 4) * 1e4 as int32, evaluated on the device."""
        k = np.ascontiguousarray(k, dtype=np.uint32); n = np.ascontiguousarray(n, dtype=np.uint32)
        out = np.zeros(len(k), np.int32)
        if len(k):
            _lib.check(self._lib.lsg_betabinom_sf4(self._h, len(k), _ptr(k), _ptr(n), float(alpha), float(beta), _ptr(out)), "lsg_betabinom_sf4")
        return out

    def betabinom_sf(self, k, n, alpha: float, beta: float):
        """(round(p, 4) * 1e4 as int32, p as float64) with p = betabinom.sf(k - 0.001, n, alpha, beta) evaluated on the device"""
        k = np.ascontiguousarray(k, dtype=np.uint32); n = np.ascontiguousarray(n, dtype=np.uint32)
        out = np.zeros(len(k), np.int32); raw = np.zeros(len(k), np.float64)
        if len(k):
            _lib.check(self._lib.lsg_betabinom_sf(self._h, len(k), _ptr(k), _ptr(n), float(alpha), float(beta), _ptr(out), _ptr(raw)), "lsg_betabinom_sf")
        return out, raw

    # ---- the beta-binomial fit (csrc/bbfit.hip; longsom_amd/bbfit.py states the arithmetic) -----
    def bbfit_reset(self, capacity: int) -> None:
        """zero the fit's six histograms (Alt_CC, Ref_CC, NC, Alt_BC, Ref_BC, DP) of `capacity` bins each"""
        _lib.check(self._lib.lsg_bbfit_reset(self._h, int(capacity)), "lsg_bbfit_reset")
        self._bbfit_cap = int(capacity)

    def bbfit_accumulate(self, ct: int, ref=None, table: int = 0, sample_n: int = 0, seed: int = 1992):
        """one pass over cell type ct's resident count rows; ref: the rows' REF bytes in genomic order (a table's own column) instead
        of the loaded reference.  Returns (rows the thinning left, rows kept of them)."""
        r = None if ref is None else np.ascontiguousarray(ref, dtype=np.uint8)
        if r is not None and len(r) != self._n_rows[ct]:
            raise ValueError("bbfit_accumulate: %d REF bytes for %d rows" % (len(r), self._n_rows[ct]))
        seen, kept = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.lsg_bbfit_accumulate(self._h, int(ct), _ptr(r), int(table), int(sample_n),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(seen), C.byref(kept)), "lsg_bbfit_accumulate")
        return int(seen.value), int(kept.value)

    def bbfit_fetch(self) -> np.ndarray:
        hist = np.zeros((6, self._bbfit_cap), np.uint64)
        _lib.check(self._lib.lsg_bbfit_fetch(self._h, _ptr(hist)), "lsg_bbfit_fetch")
        return hist

    def bbfit_add(self, hist) -> None:
        hist = np.ascontiguousarray(hist, dtype=np.uint64)
        if hist.shape != (6, self._bbfit_cap):
            raise ValueError("bbfit_add: histograms of shape %s for a capacity of %d" % (hist.shape, self._bbfit_cap))
        _lib.check(self._lib.lsg_bbfit_add(self._h, _ptr(hist)), "lsg_bbfit_add")

    def bbfit_solve(self, max_iter: int = 0):
        """([alpha1, beta1, alpha2, beta2], [info of the cell counts' fit, info of the base counts' fit]); info as bbfit.solve gives it"""
        est = np.zeros(4, np.float64)
        info = _lib.BbfitInfo()
        _lib.check(self._lib.lsg_bbfit_solve(self._h, _ptr(est), C.byref(info), int(max_iter)), "lsg_bbfit_solve")
        return [float(x) for x in est], [dict(iterations=int(info.iterations[f]), status=int(info.status[f]), last_step=float(info.last_step[f]),
                                              grad_norm=float(info.grad_norm[f])) for f in range(2)]

    def probe_posset_device(self, kind: int, keys_ptr: int, n: int, hits_ptr: int) -> None:
        """membership of n device-resident int64 keys in set `kind`, hits (uint8) written to device memory (both caller-owned)"""
        _lib.check(self._lib.lsg_probe_posset(self._h, kind, C.c_void_p(int(keys_ptr)), int(n), C.c_void_p(int(hits_ptr)), 1), "lsg_probe_posset")

    def probe_posset(self, kind: int, keys) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        hits = np.zeros(len(keys), np.uint8)
        if len(keys):
            _lib.check(self._lib.lsg_probe_posset(self._h, kind, _ptr(keys), len(keys), _ptr(hits), 0), "lsg_probe_posset")
        return hits
