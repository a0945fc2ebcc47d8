"""The SNV chain as one fused run: BAM + barcodes.tsv + reference in, the rule outputs of
SplitBam -> BaseCellCounter -> MergeCounts -> BaseCellCalling_step1/2/3 out (R:SNVCalling.smk:4-221).

The reads are decoded once and stay in HBM; the per-cell-type split is a table lookup on the device,
the merge is fused into the call kernel; only text formatting and steps 2/3 (candidate rows only) run
on the host.  Every output file has the name and the bytes the reference's scripts give it (except
the wall-clock ##fileDate line).
"""
import dataclasses
import itertools
import json
import os
import shutil
import sys
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import pandas as pd

from . import bbfit, calling, genecounts, hostio, pon, regions, tsvio
from ._lib import CallParams, CountParams
from . import _lib
from .engine import Engine


@dataclass
class SnvParams:
    """config/config.yaml:73-90 (SNVCalling block) + the script defaults the rules do not override."""
    min_mapping_quality: int = 60
    min_bq: int = 20
    min_dp: int = 5
    min_cc: int = 5
    max_depth: int = 200000                # bam.pileup(..., max_depth = 200000), BaseCellCounter.py:191 (hard-coded there)
    min_cell_types: int = 2
    min_cells: int = 5                     # BaseCellCalling.step1.py --min_cells (the PoN rules set 1)
    min_distance: int = 0
    max_gnomad_vaf: float = 0.01
    delta_vaf: float = 0.05
    delta_mcf: float = 0.3
    min_ac_reads: int = 3
    min_ac_cells: int = 2
    clust_dist: int = 10000
    alpha1: float = 0.21356677091082193
    beta1: float = 104.95163748636298
    alpha2: float = 0.2474528917555431
    beta2: float = 162.03696139428595
    reference_gz_compat: bool = False      # True reproduces SURVEY quirk Q1 (.gz position sets read as empty)
    row_digests: bool = False              # also hash the count rows as they come back from the device (SnvOutputs.row_digests; bench.py checks them against the CPU oracle's)

    def count(self) -> CountParams:
        return CountParams.longsom_defaults(min_bq=self.min_bq, min_mq=self.min_mapping_quality, min_dp=self.min_dp, min_cc=self.min_cc,
                                            max_depth=self.max_depth)

    def call(self) -> CallParams:
        return CallParams.longsom_defaults(alpha1=self.alpha1, beta1=self.beta1, alpha2=self.alpha2, beta2=self.beta2,
                                           min_ac_cells=self.min_ac_cells, min_ac_reads=self.min_ac_reads,
                                           min_cell_types=self.min_cell_types, min_cells=self.min_cells)


@dataclass
class HccvRequest:
    """run_chain(hccv=...): HighConfidenceCancerVariants.py's arguments, for the filter made on the device while the step-2 text is resident"""
    out_prefix: str
    min_dp: float = 20
    delta_vaf: float = 0.1
    delta_mcf: float = 0.4
    clust_dist: int = 10000


@dataclass
class SnvOutputs:
    report: str
    counts: Dict[str, str]
    merged: str
    step1: str
    step2: str
    step3: str
    step3_unfiltered: str
    timings: Dict[str, float] = field(default_factory=dict)
    row_digests: Optional[dict] = None     # SnvParams.row_digests: rows, columns and xxhash of (keys, reference bases, counters) per cell type, as tools/oracle_hashes.py writes them
    _pending: list = field(default_factory=list, repr=False, compare=False)
    resident: Optional[dict] = field(default=None, repr=False, compare=False)      # a rank's region and decode summary (sharded two-pass loop)
    hccv: str = ""                         # run_chain(hccv=...): the .HCCV.tsv the device made from the resident step-2 text ("": it made none)
    hccv_report: Optional[dict] = field(default=None, repr=False, compare=False)      # ... and reanno.hccv_filter_device's report of that call
    step3_report: Optional[dict] = field(default=None, repr=False, compare=False)     # calling.step3_device's report, where step 3 ran over the resident rows
    step3_path: str = ""                   # ... and the path step 3 took there: "device-resident" or "host" (not in timings: those are seconds, all of them)

    @classmethod
    def under(cls, out_dir: str, sample_id: str, celltype_names, last: str = "step3", make_dirs: bool = False) -> "SnvOutputs":
        """The files of a run under out_dir as the rules name them, up to the `last` it writes: "report", "step1" (with the count and merged
        tables), "step2" or "step3" (with the unfiltered table); the later ones stay "".  make_dirs: their four directories are made."""
        d = {k: os.path.join(out_dir, k) for k in ("SplitBam", "BaseCellCounter/" + sample_id, "MergeCounts", "BaseCellCalling")}
        if make_dirs:
            for p in d.values():
                os.makedirs(p, exist_ok=True)
        upto = ("report", "step1", "step2", "step3").index(last)
        step = lambda name: os.path.join(d["BaseCellCalling"], "%s.calling.%s.tsv" % (sample_id, name))
        out = cls(report=os.path.join(d["SplitBam"], sample_id + ".report.txt"), counts={}, merged="", step1="", step2="", step3="", step3_unfiltered="")
        if upto >= 1:
            out.counts = {name: os.path.join(d["BaseCellCounter/" + sample_id], "%s.%s.tsv" % (sample_id, name)) for name in celltype_names}
            out.merged = os.path.join(d["MergeCounts"], sample_id + ".BaseCellCounts.AllCellTypes.tsv")
            out.step1 = step("step1")
        if upto >= 2:
            out.step2 = step("step2")
        if upto >= 3:
            out.step3, out.step3_unfiltered = step("step3"), step("step3.unfiltered")
        return out

    def start_background(self, fn) -> None:
        """run fn() (table writers) on a thread of its own; wait_for_tables joins it and re-raises what it raised"""
        import threading
        box = {}

        def work():
            try:
                fn()
            except BaseException as e:                   # noqa: BLE001 — handed to the joining thread
                box["error"] = e
        th = threading.Thread(target=work, name="longsom-tables")
        th.start()
        self._pending.append((th, box))

    def wait_for_tables(self) -> float:
        t0 = time.time()
        pending, self._pending = self._pending, []
        for th, box in pending:
            th.join()
        for th, box in pending:
            if "error" in box:
                raise box["error"]
        return time.time() - t0


def write_report(path: str, report: Dict[str, int], seconds: float) -> None:
    """{id}.report.txt of SplitBamCellTypes (:181-187): one-row tab-separated table."""
    d = dict(report); d["Total_time"] = round(seconds, 2)
    pd.DataFrame([d]).to_csv(path, index=False, sep="\t")


@dataclass
class Resident:
    """One sample decoded once and resident on the GPU: contigs, reference, reads; the barcode table is swapped per pass."""
    engine: Engine
    dec: "hostio.DecodedBam"
    table: "hostio.BarcodeTable"           # the table the BAM was decoded against (dense barcode ids)
    contig_names: List[str]
    seconds: Dict[str, float]


SplitFilters = hostio.SplitFilters
REPORT_KEYS = ("total_reads", "pass_reads", "cb_not_found", "cb_not_matched", "mapq_filtered")      # lsg_bam_info's SplitBam counters, split_report's order

PILEUP_MAX_DEPTH = 200000   # bam.pileup(..., max_depth = 200000), BaseCellCounter.py:191 / HCCVSingleCellGenotype.py:122


def load_sample(bam: str, barcodes_tsv: str, ref_fasta: str, engine: Engine, min_mapq: int, allow_depth_overflow: Optional[bool] = None,
                ingest: Optional[str] = None, count_params: Optional[CountParams] = None, keep_store: bool = True, keep_unlisted: bool = False,
                filters: Optional[SplitFilters] = None) -> Resident:
    """count_params: the parameters of the count that follows, when the caller knows them (every fused rule does): the load then makes
    that count in the pass that builds the store (Engine.set_count_at_load) and the first pileup_count under them costs nothing.
    keep_store=False (with count_params): that count is the only one the caller will ask for - the load writes no tile store
    (Engine.set_store_policy); another count or a genotyping pass on these reads then raises.
    keep_unlisted: the reads without a listed barcode stay resident (never counted): the per-cell genotyping's pileup of the unsplit BAM
    holds them in its max_depth buffer (HCCVSingleCellGenotype.py:121-122); the chains that genotype pass True.
    ingest: "device" = the BAM's bytes go to the GPU and are inflated, decoded and laid out there (lsg_load_bam); "host" = the host
    decoder (liblongsom_io) + lsg_load_reads; "auto" (default, or LONGSOM_INGEST) = device, and host for a BAM whose records are not
    aligned to its BGZF blocks (not written by htslib).  Same store, same report either way (tests/test_ingest_gpu.py).
    filters: SplitBam's --max_nM / --max_NH / --n_trim (SplitFilters; None = off) - the reads they refuse are never counted, trimmed
    qualities are 0, the report gains their columns (SplitBamCellTypes.py:92-173)."""
    old_keep = hostio.set_keep_unlisted(keep_unlisted)
    try:
        # (a caller's own engine keeps the load filter / store policy it came with: Engine.loading puts them back)
        with engine.loading(count=count_params, keep_store=keep_store, keep_unlisted=keep_unlisted, filters=filters):
            return _load_sample(bam, barcodes_tsv, ref_fasta, engine, min_mapq, _ingest(ingest), filters)
    finally:
        hostio.set_keep_unlisted(old_keep)


def _load_sample(bam: str, barcodes_tsv: str, ref_fasta: str, engine: Engine, min_mapq: int, ingest: str, filters: Optional[SplitFilters] = None) -> Resident:
    t = {}
    t0 = time.time()
    bc = hostio.read_barcodes(barcodes_tsv)
    seq_of = dict(zip(*tsvio.read_fasta(ref_fasta)))
    if ingest in ("device", "auto"):
        names, lens, first = hostio.bam_header(bam)
        t["header_fasta"] = time.time() - t0
        t0 = time.time()
        _bind_reference(engine, names, lens, seq_of, ref_fasta, bc.celltype_of, len(bc.celltype_names))
        engine.set_region()
        t["reference"] = time.time() - t0
        t0 = time.time()
        got = _device_load(ingest, lambda: engine.load_bam(bam, bc.barcodes, min_mapq=min_mapq, first_record_offset=first))
        if got is not None:
            info, cb_pass, cb_low = got
            dec = _decoded(names, lens, info, [engine.split_reasons()], cb_pass, cb_low)
            t["decode"] = time.time() - t0                 # device ingest: H2D + inflate + decode + store build (info has the phases)
            t["load"] = 0.0
            for k, v in info.items():                      # the phases of the device ingest, in seconds like everything else here
                if k.startswith("ms_") and k != "ms_total":
                    t["ingest_" + k[3:]] = float(v) / 1e3
            return Resident(engine, dec, bc, names, t)
        t0 = time.time()
    dec = hostio.decode_bam(bam, bc.barcodes, min_mapq=min_mapq, filters=filters)
    t["decode"] = time.time() - t0
    t0 = time.time()
    # the pileup is driven by the FASTA's contigs (MakeWindows, BaseCellCounter.py:84-86); BAM tids index dec.contig_names
    _bind_reference(engine, dec.contig_names, dec.contig_len, seq_of, ref_fasta, bc.celltype_of, len(bc.celltype_names))
    engine.set_region()
    engine.load_reads(dec.records)
    t["load"] = time.time() - t0
    return Resident(engine, dec, bc, dec.contig_names, t)


def _ingest(mode: Optional[str] = None) -> str:
    """how a BAM's reads reach the GPU (load_sample's `ingest`): the caller's choice, else LONGSOM_INGEST, else auto"""
    return mode or os.environ.get("LONGSOM_INGEST", "auto")


def _straddles(e: BaseException) -> bool:
    """the device ingest refused a BAM whose records are not aligned to its BGZF blocks (not written by htslib)"""
    return isinstance(e, _lib.LsgError) and "straddle" in str(e)


def _device_load(ingest: str, load):
    """load() - an ingest on the device - or None when the device refused a BAM whose records straddle its blocks and `ingest` ("auto")
    leaves such a BAM to the host decoder"""
    try:
        return load()
    except _lib.LsgError as e:
        if ingest == "device" or not _straddles(e):
            raise
        return None


def _bind_reference(eng: Engine, names, lens, seq_of: dict, ref_fasta: str, celltype_of, n_celltypes: int) -> None:
    """the BAM's contigs - every one in the FASTA, with the same length - and their sequences on the device, then the barcode table"""
    for n, l in zip(names, lens):
        if n not in seq_of or len(seq_of[n]) != int(l):
            raise ValueError("contig %s of the BAM header is missing from %s or has another length" % (n, ref_fasta))
    eng.set_contigs(lens)
    for tid, n in enumerate(names):
        eng.load_reference(tid, seq_of[n])
    eng.set_barcodes(celltype_of, n_celltypes)


def _decoded(names, lens, info, reasons, cb_pass=None, cb_low=None) -> "hostio.DecodedBam":
    """a device ingest's DecodedBam: no records; the report from its counters (lsg_bam_info) and its loads' Engine.split_reasons"""
    rep = hostio.split_report([info[k] for k in REPORT_KEYS], reasons)
    return hostio.DecodedBam(None, names, np.asarray(lens, np.int64), rep, None, cb_pass, cb_low)


def chain_step1(res: Resident, celltype_of: np.ndarray, celltype_names: List[str], report: Dict[str, int], out_dir: str, sample_id: str,
                params: SnvParams, write_tables: bool = True, background_tables: bool = False, kept_rows: bool = True, last: str = "step1"):
    """SplitBam report -> BaseCellCounter -> MergeCounts -> BaseCellCalling step 1 over the resident reads.  Returns (outputs, text of
    the rows step 2 keeps, call records, timings); write_tables=False keeps everything off the disk except the report.  last: the last
    table the caller writes (SnvOutputs.under): the outputs name its file and those before it."""
    eng, contig_names = res.engine, res.contig_names
    t = dict(res.seconds)
    t0 = time.time()
    eng.set_barcodes(celltype_of, len(celltype_names))
    n_rows, n_cols = eng.pileup_count(params.count())
    n_sites, n_cand = eng.call_step1(params.call())
    t["gpu_count_call"] = time.time() - t0
    t0 = time.time()
    out = SnvOutputs.under(out_dir, sample_id, celltype_names, last if write_tables else "report", make_dirs=True)
    write_report(out.report, report, t["decode"])
    if not write_tables:
        calls = eng.fetch_calls(candidates_only=True)
        t["fetch"] = time.time() - t0
        return out, None, calls, t
    date = tsvio.file_date()
    if os.environ.get("LONGSOM_HOST_TABLES", "0") != "1":
        return _device_tables(eng, out, contig_names, celltype_names, sample_id, params, date, background_tables, t, t0, (n_rows, n_cols, n_sites, n_cand), kept_rows)
    import threading
    per_ct: List = [None] * len(celltype_names)
    arrived = [threading.Event() for _ in celltype_names]          # a cell type's count rows are on the host
    failed: List[BaseException] = []                               # ... or will never be

    def count_tables():
        for ct, name in enumerate(celltype_names):
            arrived[ct].wait()
            if failed:
                return
            t1 = time.time()
            tsvio.write_counts_tsv(out.counts[name], *per_ct[ct], contig_names, "%s.%s" % (sample_id, name), date)
            t["table_counts_" + name] = time.time() - t1        # (seconds of the writer itself, in the background when background_tables)

    def merged_table():
        if failed:
            return
        t1 = time.time()
        tsvio.write_merged_tsv(out.merged, per_ct, contig_names, celltype_names, date)
        t["table_merged"] = time.time() - t1
    try:
        for ct in range(len(celltype_names)):
            per_ct[ct] = eng.fetch_counts(ct)
            arrived[ct].set()
            if ct == 0 and background_tables:
                # the per-cell-type and the merged table need the count rows only: their writer starts with the first cell type's rows, while
                # the others' and the call records are still on their way from the device (the merged table behind the count tables on ONE
                # thread: a third writer beside steps 2 and 3 made every one of them slower - the host's threads are all busy - and the run
                # no shorter)
                out.start_background(lambda: (count_tables(), merged_table()))
    except BaseException as e:                                   # (the writer must not wait for rows that will never come)
        failed.append(e)
        for ev in arrived:
            ev.set()
        raise
    calls = eng.fetch_calls()
    t["fetch"] = time.time() - t0
    if params.row_digests:
        t0 = time.time()
        out.row_digests = _row_digests(eng, len(celltype_names), (n_rows, n_cols, n_sites, n_cand), per_ct)
        t["row_digests"] = time.time() - t0
    t0 = time.time()
    header = tsvio.merged_comment_lines(date)
    if background_tables:
        # Steps 2 and 3 only need the rows step 2 keeps: those are formatted first (a third of the step-1 table's rows, nothing written);
        # the per-cell-type and merged tables and the step-1 table itself are written by threads of their own (native writers, no GIL)
        # beside steps 2 and 3 - the box's disk takes several files at once faster than one: the caller joins them (SnvOutputs.wait_for_tables)
        s1 = tsvio.step1_kept_rows(calls, per_ct, contig_names, celltype_names, header, as_bytes=True)
        def step1_table():
            t1 = time.time()
            tsvio.write_step1_tsv(out.step1, calls, per_ct, contig_names, celltype_names, header, collect=False)
            t["table_step1"] = time.time() - t1
        out.start_background(step1_table)
        t["write_tables"] = time.time() - t0          # (what the chain waited for: the kept rows; tables_wait is what was left of the writers at the end)
        return out, s1, calls, t
    count_tables()
    merged_table()
    s1 = tsvio.write_step1_tsv(out.step1, calls, per_ct, contig_names, celltype_names, header, as_bytes=True)      # s1 = header + the rows step 2 keeps
    t["write_tables"] = time.time() - t0
    return out, s1, calls, t


def _row_digests(eng, n_ct: int, shape, per_ct=None) -> dict:
    """SnvParams.row_digests: rows, columns and xxhash of (keys, reference bases, counters) per cell type, as tools/oracle_hashes.py writes them"""
    import xxhash
    n_rows, n_cols, n_sites, n_cand = shape
    out = {"rows": [int(x) for x in n_rows], "columns": int(n_cols), "merged_sites": int(n_sites), "candidate_rows": int(n_cand)}
    for ct in range(n_ct):
        rows = per_ct[ct] if per_ct is not None else eng.fetch_counts(ct)
        out["ct%d" % ct] = [xxhash.xxh64(np.ascontiguousarray(x).tobytes() if x.size < (1 << 20) else memoryview(np.ascontiguousarray(x)).cast("B")).hexdigest() for x in rows]
    return out


def _device_tables(eng, out: "SnvOutputs", contig_names, celltype_names, sample_id, params, date, background: bool, t, t0, shape, kept_rows: bool = True):
    """The tables of chain_step1 printed on the device (Engine.format_table: csrc/tables.hip, byte for byte the host writers' text) and
    streamed into their files (Engine.append_table), one thread per file; the count rows never come to the host.  The rows step 2 keeps
    come first - steps 2 and 3 wait for nothing else.  LONGSOM_HOST_TABLES=1 keeps the host writers (csrc/hostio/tsvwrite.cpp)."""
    import threading
    eng.set_table_names(contig_names, celltype_names)
    head1 = tsvio.step1_head(celltype_names, date)
    s1 = head1.encode()
    if kept_rows:                                    # (kept_rows=False: the caller runs step 2 on the device too and wants the header alone)
        n = eng.format_table(eng.TABLE_STEP1_KEPT)
        s1 = eng.table_bytes(eng.TABLE_STEP1_KEPT, n, prefix=s1)
        eng.free_table(eng.TABLE_STEP1_KEPT)
    t["fetch"] = time.time() - t0                    # (what came to the host: the kept rows' text)
    t0 = time.time()
    files = [(ct, out.counts[name], tsvio.counts_header("%s.%s" % (sample_id, name), date)) for ct, name in enumerate(celltype_names)]
    files += [(eng.TABLE_MERGED, out.merged, tsvio.merged_header(celltype_names, date)), (eng.TABLE_STEP1, out.step1, head1)]
    sizes = {}
    for table, path, head in files:
        with open(path, "w") as f:
            f.write(head)
        sizes[table] = eng.format_table(table)
    t["format_tables"] = time.time() - t0
    t0 = time.time()

    def stream(table, path):
        t1 = time.time()
        eng.append_table(table, path)
        eng.free_table(table)
        t["table_%d" % table] = time.time() - t1
    if background:
        for table, path, _ in files:                  # (the box's file system takes several files at once faster than one)
            out.start_background(lambda table=table, path=path: stream(table, path))
    else:
        for table, path, _ in files:
            stream(table, path)
    t["write_tables"] = time.time() - t0
    if params.row_digests:
        t1 = time.time()
        out.row_digests = _row_digests(eng, len(celltype_names), shape)
        t["row_digests"] = time.time() - t1
    calls = None if background else eng.fetch_calls()
    return out, s1, calls, t


def run_chain(res: Resident, celltype_of: np.ndarray, celltype_names: List[str], report: Dict[str, int], out_dir: str, sample_id: str,
              params: SnvParams, editing: Optional[str] = None, pon_sr: Optional[str] = None, pon_lr: Optional[str] = None,
              gnomad_af_json: Optional[str] = None, step3: bool = True, hccv: Optional[HccvRequest] = None) -> SnvOutputs:
    """SplitBam report -> BaseCellCounter -> MergeCounts -> BaseCellCalling step 1-3 for one barcode -> cell-type table over the
    resident reads (celltype_of[barcode id] = index into celltype_names, 255 = barcode not listed).  step3=False stops after
    step 2, as pass 1 of the reference does (rules/CellTypeReannotation.smk has no step-3 rule: HCCV reads calling.step2.tsv).
    hccv: where the device prints the step-2 table itself, the high-confidence cancer variant filter runs over that text while it is
    resident (SnvOutputs.hccv names its file; "" when this run's step 2 was the host's, or the table is one for reanno.hccv_filter)."""
    eng, contig_names = res.engine, res.contig_names
    # Step 2 with --min_distance 0 (LongSom's own setting) tags rows by position sets and by gnomAD alleles and blanks NA cells: the device
    # prints that table itself and tells step 3 what it needs of it (_device_steps23); any other step 2 - a distance filter, a
    # --gnomAD_max <= 0 (the reference then tags every row, whatever the database holds), contigs beyond the allele key's limits - runs on
    # the host over the text of the rows it keeps.  LONGSOM_HOST_TABLES=1 / LONGSOM_HOST_STEP2=1 keep the host paths.  The gnomAD source
    # is opened first: one that cannot be used stops the run before anything is counted (calling.open_gnomad).
    gnomad = calling.open_gnomad(gnomad_af_json)
    if isinstance(gnomad, calling.GnomadSet):
        gnomad.require(params.max_gnomad_vaf)
    device23 = (os.environ.get("LONGSOM_HOST_TABLES", "0") != "1" and os.environ.get("LONGSOM_HOST_STEP2", "0") != "1"
                and int(params.min_distance) == 0 and len(set(contig_names)) == len(contig_names)
                and not any(ch in n for n in list(contig_names) + list(celltype_names) for ch in "\t\n")
                and (not gnomad or (params.max_gnomad_vaf > 0 and calling.allele_keys_fit(eng.contig_len) and calling.keyed_by_alleles(gnomad))))
    out, s1, _, t = chain_step1(res, celltype_of, celltype_names, report, out_dir, sample_id, params, background_tables=True, kept_rows=not device23,
                                last="step3" if step3 else "step2")
    try:
        if device23:
            return _device_steps23(out, s1, t, eng, contig_names, params, editing, pon_sr, pon_lr, step3, gnomad, hccv)
        return _chain_steps23(out, s1, t, eng, contig_names, params, editing, pon_sr, pon_lr, gnomad, step3)
    except BaseException:
        try:                                   # (the writers stream from the engine: nobody may close it under them)
            out.wait_for_tables()
        except BaseException:                  # noqa: BLE001 - the first error is the one to report
            pass
        raise


def _device_steps23(out, head1: bytes, t, eng, contig_names, params, editing, pon_sr, pon_lr, step3, gnomad=None, hccv=None):
    """Steps 2 and 3 of run_chain with the step-2 table printed on the device (Engine.TABLE_STEP2: csrc/tables.hip): its text goes from
    the device straight into its file; the host sees the kinds of cell of its columns and the rows step 3 can keep
    (Engine.step2_summary), which is all calling.step3 reads of a table this large.  gnomad (calling.open_gnomad's): the alleles it tags
    are resident while the table is printed - a prepared set's as they are, a database's or a JSON table's after it was asked about the
    one-base alleles this run holds (Engine.step2_allele_queries) and nothing else."""
    t0 = time.time()
    for kind, k in zip((calling.KIND_EDITING, calling.KIND_PON_SR, calling.KIND_PON_LR), _posset_keys(contig_names, params, editing, pon_sr, pon_lr)):
        eng.load_posset(kind, k)
    hdr = calling.step2_head(head1)                 # (the table's head as step 2 writes it)
    cols = hdr.decode().split("\n")[-2].split("\t")
    with open(out.step2, "wb") as f:
        f.write(hdr)
    if gnomad:
        t1 = time.time()
        if isinstance(gnomad, calling.GnomadSet):
            hits = gnomad.hit_keys(contig_names, params.max_gnomad_vaf)
        else:
            hits = calling.gnomad_hit_keys(gnomad, contig_names, eng.step2_allele_queries(), params.max_gnomad_vaf)
        eng.load_alleleset(hits)
        t["step2_gnomad"] = time.time() - t1          # (part of step2: the source's answers and the set's load)
    try:
        n2 = eng.format_table(eng.TABLE_STEP2)
    finally:
        eng.load_alleleset(None)                      # (a later run on this engine without a source must not be tagged)
    kinds, n_surv = eng.step2_summary(len(cols))
    if not step3:
        eng.free_table(eng.TABLE_STEP3_ROWS)
    out.start_background(lambda: eng.append_table(eng.TABLE_STEP2, out.step2))
    t["step2"] = time.time() - t0
    if hccv is not None:
        # the filter between the two passes of the re-annotation, over the same resident text (the table's file is still being written:
        # a table the row code does not decide is left to the caller, who runs reanno.hccv_filter once the file is whole)
        from . import reanno
        t1 = time.time()
        out.hccv_report = {}
        os.makedirs(os.path.dirname(hccv.out_prefix) or ".", exist_ok=True)
        out.hccv = reanno.hccv_filter_device(eng, out.step2, hccv.out_prefix, hccv.min_dp, hccv.delta_vaf, hccv.delta_mcf, hccv.clust_dist, resident=True, head=hdr,
                                             kinds=kinds, fallback=False, report=out.hccv_report) or ""
        t["hccv_device"] = time.time() - t1
    try:
        if step3:
            _device_step3(out, eng, hdr, kinds, n_surv, n2, params, t)
        t["tables_wait"] = out.wait_for_tables()
    finally:
        try:
            out.wait_for_tables()
        finally:
            for table in (eng.TABLE_STEP2, eng.TABLE_STEP3_ROWS, eng.TABLE_STEP3_ALL, eng.TABLE_STEP3_PASS):
                eng.free_table(table)
    out.timings = t
    return out


def _device_step3(out, eng, hdr: bytes, kinds, n_surv: int, n2: int, params, t) -> None:
    """Step 3 of _device_steps23 over the rows step2_summary left resident (Engine.TABLE_STEP3_ROWS): decided and printed on the device
    (calling.step3_device), the final table written here and the unfiltered one streamed into its file by the background writers.  Those
    rows come to the host only when the row code hands the table back - or with LONGSOM_HOST_STEP3=1 -, for calling.step3 as before.
    out.step3_path: "device-resident", or "host"."""
    t0 = time.time()
    done, out.step3_report = None, {}
    if os.environ.get("LONGSOM_HOST_STEP3", "0") != "1":
        done = calling.step3_device(eng, None, out.step3, out.step3_unfiltered, params.delta_vaf, params.delta_mcf, params.min_ac_reads, params.min_ac_cells,
                                    params.clust_dist, resident=True, head=hdr, kinds=kinds, report=out.step3_report, background=out.start_background)
    if done is None:
        survivors = eng.table_bytes(eng.TABLE_STEP3_ROWS, n_surv, prefix=hdr)
        eng.free_table(eng.TABLE_STEP3_ROWS)
        _write_step3(out, survivors, params, t, all_kinds=kinds, full_text=lambda: eng.table_bytes(eng.TABLE_STEP2, n2, prefix=hdr), survivors_only=True)
    t["step3"] = time.time() - t0
    out.step3_path = out.step3_report["path"] if done is not None else "host"


def _chain_steps23(out, s1, t, eng, contig_names, params, editing, pon_sr, pon_lr, gnomad, step3):
    t0 = time.time()
    s2 = _step2_for(eng, contig_names, params, editing, pon_sr, pon_lr, None, gnomad)(s1, params.min_distance)
    tsvio.write_bytes(out.step2, s2)
    t["step2"] = time.time() - t0
    if step3:
        _write_step3(out, s2, params, t)
    t["tables_wait"] = out.wait_for_tables()              # (what of the background writers' time steps 2 and 3 did not cover)
    out.timings = t
    return out


def _posset_keys(contig_names, params: SnvParams, editing, pon_sr, pon_lr) -> list:
    """the keys of step 2's position sets over the run's contigs: RNA editing, PoN_SR, PoN_LR"""
    return [calling.read_posset_keys(p, contig_names, params.reference_gz_compat) for p in (editing, pon_sr, pon_lr)]


def _step2_for(eng, contig_names, params: SnvParams, editing, pon_sr, pon_lr, gnomad_af_json, gnomad=None):
    """step 2 of one run: (text of a step-1 table, distance) -> text of the step-2 table.  The position sets are read and the gnomAD source
    (a JSON table, a gnomad_db directory / sqlite file or a prepared set; or, as `gnomad`, one the caller opened) is opened here, once:
    one that cannot be used stops the run (calling.open_gnomad)."""
    ed, sr, lr = _posset_keys(contig_names, params, editing, pon_sr, pon_lr)
    af = gnomad if gnomad is not None else calling.open_gnomad(gnomad_af_json)
    return lambda text, distance: calling.step2_bytes(text, eng, contig_names, ed, sr, lr, distance, af, params.max_gnomad_vaf)


def _write_step3(out: SnvOutputs, s2: bytes, params: SnvParams, t, **kw) -> None:
    """step 3 over the text of the step-2 table (or what of it step 3 reads: calling.step3's all_kinds / full_text / survivors_only in kw)
    into its two files"""
    t0 = time.time()
    final, unfiltered = calling.step3_bytes(s2, params.delta_vaf, params.delta_mcf, params.min_ac_reads, params.min_ac_cells, params.clust_dist, **kw)
    tsvio.write_bytes(out.step3, final)
    tsvio.write_bytes(out.step3_unfiltered, unfiltered)
    t["step3"] = time.time() - t0


def run_snv(bam: str, barcodes_tsv: str, ref_fasta: str, out_dir: str, sample_id: str, params: Optional[SnvParams] = None,
            editing: Optional[str] = None, pon_sr: Optional[str] = None, pon_lr: Optional[str] = None,
            gnomad_af_json: Optional[str] = None, device: int = 0, engine: Optional[Engine] = None,
            comm: Optional["regions.Comm"] = None, window_bytes: Optional[int] = None, filters: Optional[SplitFilters] = None,
            gene_counts: Optional["genecounts.Request"] = None) -> SnvOutputs:
    """One sample through the whole chain.  comm (world > 1): one rank per GPU, genomic regions sharded over the ranks, call
    `regions.Comm.from_env()` before anything touches the GPU.  window_bytes: stream the BAM in batches of about that many
    uncompressed bytes and count window by window (a BAM whose reads do not fit in HBM; decode overlaps the GPU work).  filters: SplitBam's
    --max_nM / --max_NH / --n_trim (SplitFilters; None = off), applied by every form of the ingest.  gene_counts (a genecounts.Request):
    the cell-by-gene read counts of the CNA branch are made from the same load before the chain runs (rules/CNACalling.gpu.smk); the load
    then keeps every record (no load filter), and sharded or windowed runs refuse it: a read that reaches into two regions would count twice."""
    params = params or SnvParams()
    comm = comm or regions.Comm()
    if gene_counts is not None and (comm.world > 1 or window_bytes):
        raise ValueError("gene_counts needs the whole BAM resident at once: a read that reaches into two regions of a sharded (%d ranks) or windowed "
                         "(--window_gb) run would be counted twice; run cli.gene_counts on its own" % comm.world)
    own = engine is None
    eng = engine or Engine(comm.local_device_index if comm.world > 1 else device)
    try:
        if comm.world > 1 and window_bytes:
            raise ValueError("window_bytes (--window_gb) streams one process's BAM window by window; with %d ranks every rank holds its region's reads at once: "
                             "use one or the other" % comm.world)
        if comm.world > 1 or window_bytes:
            return _run_snv_regions(bam, barcodes_tsv, ref_fasta, out_dir, sample_id, params, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm, window_bytes, keep_store=not own,
                                    filters=filters)
        # (the chain counts its sample once: an engine of our own keeps no store for counts nobody will ask for)
        # (... unless the gene counts read the load as well: a load without a store drops the reads its one count refuses)
        res = load_sample(bam, barcodes_tsv, ref_fasta, eng, params.min_mapping_quality, count_params=params.count(), keep_store=not own or gene_counts is not None,
                          filters=filters)
        if gene_counts is not None:
            genecounts.run_resident(eng, res.contig_names, res.table.barcodes, gene_counts, sample_id)
        return run_chain(res, res.table.celltype_of, res.table.celltype_names, res.dec.report, out_dir, sample_id, params, editing, pon_sr, pon_lr,
                         gnomad_af_json)
    finally:
        if own:
            eng.close()


def _key(p) -> int:
    return (int(p[0]) << 32) | int(p[1])


def _windows(batches, n_contigs: int):
    """(lo, hi, records) per window from a stream of decoded batches in file (= coordinate) order: a window's region ends at the
    start tile of the next batch's first read — every read that can cover a column below that point has been seen — and the reads
    that reach past it are carried into the next window."""
    carry = None
    lo = (0, 0)
    prev = next(batches, None)
    while prev is not None:
        nxt = next(batches, None)
        while nxt is not None and nxt.records.n_reads == 0:          # a batch whose records were all dropped at decode: merge its counters forward
            for k, v in nxt.report.items():
                prev.report[k] = prev.report.get(k, 0) + v
            nxt = next(batches, None)
        rec = prev.records if carry is None else hostio.concat_records([carry, prev.records])
        hi = (n_contigs, 0)
        if nxt is not None:
            hi = (int(nxt.records.read_tid[0]), (int(nxt.records.read_pos[0]) // regions.TILE) * regions.TILE)
        if _key(hi) < _key(lo):
            raise ValueError("the BAM is not coordinate sorted: a batch starts at %s, before %s" % (hi, lo))
        yield lo, hi, rec, prev
        carry = None
        if nxt is not None and rec.n_reads:
            ends = regions.read_ends(rec)
            mask = ((rec.read_tid.astype(np.int64) << 32) | ends) > _key(hi)
            if mask.any():
                carry = rec.subset(mask)
        lo, prev = hi, nxt


def _prefetch(gen, depth: int = 1):
    """run a generator in a background thread, `depth` items ahead (the decode of the next batch overlaps the GPU and the writers)"""
    import queue
    import threading
    q: "queue.Queue" = queue.Queue(maxsize=depth)
    end = object()

    def work():
        try:
            for item in gen:
                q.put(item)
            q.put(end)
        except BaseException as e:            # noqa: BLE001 - handed to the consumer
            q.put(e)
    threading.Thread(target=work, daemon=True).start()
    while True:
        item = q.get()
        if item is end:
            return
        if isinstance(item, BaseException):
            raise item
        yield item


def _run_snv_regions(bam, barcodes_tsv, ref_fasta, out_dir, sample_id, params, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm, window_bytes,
                     step3: bool = True, resident: Optional[dict] = None, table=None, keep_store: bool = True, filters: Optional[SplitFilters] = None) -> SnvOutputs:
    """The sharded and the windowed run, in three parts: where this rank's reads come from (_region_source), the count loop over its
    windows, which writes their pieces of the tables (_count_windows), and rank 0's assembly of the pieces and steps 2-3 (_assemble).
    keep_store=False: a rank's slice is counted once and nothing else is asked of its reads (run_snv): the load keeps no tile store.
    resident / table / step3 serve the sharded two-pass loop (run_reannotation with several ranks): `resident` = SnvOutputs.resident of
    an earlier call on the same engine (the rank's reads stay in HBM, nothing is ingested again), `table` = (celltype_of per barcode
    id, cell-type names, SplitBam report) of the pass, step3=False stops after the step-2 table (pass 1 of the reference has no step 3)."""
    t: Dict[str, float] = {"decode": 0.0, "load": 0.0, "gpu_count_call": 0.0, "fetch": 0.0, "write_tables": 0.0}
    t_all = time.time()
    bc = hostio.read_barcodes(barcodes_tsv)
    seq_of = dict(zip(*tsvio.read_fasta(ref_fasta)))
    cts = list(table[1]) if table is not None else bc.celltype_names
    ct_of = np.asarray(table[0], np.uint8) if table is not None else bc.celltype_of
    out = SnvOutputs.under(out_dir, sample_id, cts, "step3" if step3 else "step2", make_dirs=comm.rank == 0)
    tmp = os.path.join(out_dir, "_pieces." + sample_id)
    if comm.rank == 0:
        shutil.rmtree(tmp, ignore_errors=True)
        os.makedirs(tmp, exist_ok=True)
    comm.barrier()
    bind = lambda names, lens: _bind_reference(eng, names, lens, seq_of, ref_fasta, ct_of, len(cts))
    names, work = _region_source(eng, bam, bc, bind, ct_of, len(cts), params, comm, window_bytes, resident, keep_store, filters, t)
    # Step 2 is row-local when its distance filter is off (LongSom's setting: min_distance 0) — position-set probes, the gnomAD lookup, the
    # FILTER tags and the blanked NA fields all look at one row — so every rank (every window) runs it over its own rows on its own GPU,
    # writes its pieces of the step-2 table, and only the rows that survive step 3's FILTER patterns travel to rank 0, whose step 3 needs
    # the candidates of every region for its cluster filter (step3.py:283-306).  With a distance filter the rows' neighbours matter and
    # rank 0 runs step 2 over all kept rows.
    local_step2 = int(params.min_distance) == 0
    new_step2 = lambda: _step2_for(eng, names, params, editing, pon_sr, pon_lr, gnomad_af_json)
    got, region_error = None, None
    try:
        got = _count_windows(eng, work, names, cts, params, tmp, new_step2 if local_step2 else None, t)
    except BaseException as e:                              # noqa: BLE001 - raised again by the vote below, on every rank
        region_error = e
    # (no collective inside the loop: a rank that failed there is heard of here, before anybody waits for its rows)
    comm.agree(region_error, "counting / writing a rank's region of %s" % bam)
    kept, kinds, report, t["windows"], last = got
    # the candidate rows of every region on every rank (RCCL all-gather over xGMI when world > 1); then the pieces are complete
    payloads = comm.allgather_bytes(regions.pack_rows(kept))
    kinds_all = None
    if local_step2:                                    # the kinds of cell every rank saw in its rows of the step-2 table, OR-ed
        for blob in comm.allgather_bytes(kinds.tobytes() if kinds is not None else b""):
            if blob:
                kinds_all = _union_kinds(kinds_all, np.frombuffer(blob, np.uint8))
    comm.barrier()
    if table is not None and table[2] is not None:     # (a pass under its own barcode table has its own SplitBam report)
        report = dict(table[2])
    if comm.rank == 0:
        _assemble(out, tmp, sample_id, cts, report, t["decode"] if comm.world > 1 else time.time() - t_all, payloads, kinds_all,
                  None if local_step2 else new_step2, params, step3, t)
    comm.barrier()
    out.timings = t
    if comm.world > 1:
        lo, hi, dec = last
        out.resident = {"lo": lo, "hi": hi, "dec": dec, "table": bc}
    return out


def _region_source(eng, bam, bc, bind, ct_of, n_ct, params, comm, window_bytes, resident, keep_store, filters, t):
    """How this rank's reads reach the GPU, decided once: (contig names, the windows the count loop takes: (lo, hi, records to load or
    None when they are loaded already, DecodedBam with the window's report)).  bind(names, lens): _bind_reference for this pass."""
    if resident is not None:
        if comm.world <= 1:
            raise ValueError("a resident pass belongs to a run with several ranks")
        return _resident_window(eng, resident, ct_of, n_ct)
    ingest = _ingest()
    if comm.world > 1:
        return _rank_region(eng, bam, bc, bind, params, comm, ingest, keep_store, filters, t)
    bai = hostio.find_bai(bam) if ingest in ("device", "auto") else None
    if bai is not None:
        return _indexed_windows(eng, bam, bai, bc, bind, params, window_bytes, filters, t)
    return _streamed_windows(bam, bc, bind, params, window_bytes, filters)


def _resident_window(eng, resident, ct_of, n_ct):
    """pass 2 of the sharded two-pass loop: the rank's reads are in HBM already, the pass differs by its barcode table only"""
    eng.set_barcodes(ct_of, n_ct)
    dec = resident["dec"]
    return dec.contig_names, [(resident["lo"], resident["hi"], None, dec)]


def _rank_region(eng, bam, bc, bind, params, comm, ingest, keep_store, filters, t):
    """One rank's region of a sharded run.  Every rank ingests the file on its OWN GPU (inflate, decode, store: 0.5 s per GB, nothing on
    the host's threads, which the ranks used to share): the slice its region needs when the BAM has an index (_rank_slice), else the
    whole file (_rank_of_whole_file).  The host decoder takes the file under host ingest, or when the device refused it (records that
    straddle its blocks); every rank then decodes all of it and loads the reads of its region."""
    t0 = time.time()
    device = ingest in ("device", "auto")
    win = None
    if device:
        names, lens, first = hostio.bam_header(bam)
        bind(names, lens)
        bai = hostio.find_bai(bam)
        if bai is not None:
            win = _rank_slice(eng, bam, bai, names, lens, bc, params, comm, keep_store, filters, t)
        if win is None:
            win = _device_load(ingest, lambda: _rank_of_whole_file(eng, bam, names, lens, first, bc, params, comm, filters))
    if win is None:
        dec = hostio.decode_bam(bam, bc.barcodes, min_mapq=params.min_mapping_quality, threads=max(1, (os.cpu_count() or 1) // comm.world), filters=filters)
        bounds = regions.balanced_boundaries(dec.records, len(dec.contig_names), comm.world)
        lo, hi = bounds[comm.rank], bounds[comm.rank + 1]
        win = (lo, hi, dec.records.subset(regions.reads_overlapping(dec.records, lo, hi)), dec)
    t["decode"] = time.time() - t0
    if device:                                         # (the header's contigs are bound already)
        return names, [win]
    return win[3].contig_names, _bound_on_arrival(bind, win[3], [win])


def _rank_slice(eng, bam, bai, names, lens, bc, params, comm, keep_store, filters, t):
    """Every rank ingests the SLICE of the file its region needs, found through the .bai's linear index (regions.BaiPlan), as the
    reference's workers fetch their window through the index; SplitBam's counters are summed over the ranks (each record is counted by the
    rank whose region holds its start).  The rank's region and the count's parameters are known before its slice is loaded: the load
    counts in the same pass (keep_store=False, run_snv: it is the slice's only count - what load_sample does for one GPU).  Any rank that
    cannot (records not aligned to the blocks of its slice) takes every rank to the whole file: the ranks agree first, and all return None."""
    plan = regions.BaiPlan(hostio.read_bai(bai), len(names), comm.world, os.path.getsize(bam))
    lo, hi = plan.bounds[comm.rank], plan.bounds[comm.rank + 1]
    got, reasons, ok, fatal = None, None, 1, None
    try:
        eng.set_region(lo[0], lo[1], hi[0], hi[1])
        with eng.loading(count=params.count(), keep_store=keep_store, filters=filters):
            got = regions.ingest_slice(eng, bam, plan, lo, hi, bc.barcodes, params.min_mapping_quality)
            reasons = eng.split_reasons() if got is not None else None
    except BaseException as e:                     # noqa: BLE001 - an index that is not this BAM's, a corrupt block, no memory ...
        ok, fatal = (0, None) if _straddles(e) else (1, e)
    comm.agree(fatal, "the ingest of a rank's slice of %s" % bam)      # (every rank raises when one did: nobody waits in the all-reduce below)
    if int(comm.allreduce_sum(np.asarray([ok], np.int64))[0]) != comm.world:
        return None
    # SplitBam's counters, the tallies, and per rank: records and bytes of its slice, its filter reasons (counts, first ordinals + 1: 0 = none)
    n_cb, R, W, r = len(bc.barcodes), hostio.N_REASONS, comm.world, comm.rank
    at_n = 5 + 2 * n_cb
    at_r = at_n + 2 * W
    counts = np.zeros(at_r + 2 * R * W, np.int64)
    if got is not None:
        info, cb_pass, cb_low = got
        counts[:5] = [info[k] for k in REPORT_KEYS]; counts[5:5 + n_cb] = cb_pass; counts[5 + n_cb:at_n] = cb_low
        counts[at_n + r] = info["n_records"]; counts[at_n + W + r] = info["slice_bytes"]
        counts[at_r + R * r:at_r + R * (r + 1)] = reasons[0]
        counts[at_r + R * (W + r):at_r + R * (W + r + 1)] = reasons[1] + 1
    else:
        eng.load_reads(hostio.ReadRecords.empty())      # (no alignment in this rank's region)
    counts = comm.allreduce_sum(counts)
    t["ingest_records_by_rank"] = counts[at_n:at_n + W].tolist()
    t["ingest_slice_MB_by_rank"] = [round(x / 1e6, 3) for x in counts[at_n + W:at_r].tolist()]
    rs = [(counts[at_r + R * q:at_r + R * (q + 1)], counts[at_r + R * (W + q):at_r + R * (W + q + 1)] - 1) for q in range(W)]
    return lo, hi, None, _decoded(names, lens, dict(zip(REPORT_KEYS, counts[:5])), rs, counts[5:5 + n_cb].copy(), counts[5 + n_cb:at_n].copy())


def _rank_of_whole_file(eng, bam, names, lens, first, bc, params, comm, filters):
    """the whole file on every rank's GPU; the regions come from its resident per-read arrays, the same on every rank (the rank's store
    holds the whole file, lsg_set_region makes its region's columns its own)"""
    with eng.loading(filters=filters):
        info, cb_pass, cb_low = eng.load_bam(bam, bc.barcodes, min_mapq=params.min_mapping_quality, first_record_offset=first)
    dec = _decoded(names, lens, info, [eng.split_reasons()], cb_pass, cb_low)
    bounds = regions.balanced_boundaries(eng.reads_to_host(events=False), len(names), comm.world)
    return bounds[comm.rank], bounds[comm.rank + 1], None, dec


def _indexed_windows(eng, bam, bai, bc, bind, params, window_bytes, filters, t):
    """windows of an INDEXED BAM: the regions a sharded run would give its ranks, taken one after the other by this one GPU — every
    window's slice of the file goes to the device as it is (regions.ingest_slice: no host decode, no carried reads: a slice holds every
    read that reaches into its region)"""
    names, lens, _ = hostio.bam_header(bam)
    n_win = max(1, -(-os.path.getsize(bam) * 3 // int(window_bytes)))          # (window_bytes counts uncompressed bytes: about a third as many in the file)
    plan = regions.BaiPlan(hostio.read_bai(bai), len(names), n_win, os.path.getsize(bam))

    def windows():
        bind(names, lens)
        for lo, hi in zip(plan.bounds, plan.bounds[1:]):
            t0 = time.time()
            with eng.loading(filters=filters):
                got = regions.ingest_slice(eng, bam, plan, lo, hi, bc.barcodes, params.min_mapping_quality)
            t["decode"] += time.time() - t0
            if got is not None:
                # (the windows' reports are summed in file order: a reason's column lands where its first window put it)
                yield lo, hi, None, _decoded(names, lens, got[0], [eng.split_reasons()])
    return names, windows()


def _streamed_windows(bam, bc, bind, params, window_bytes, filters):
    """windows of a BAM without an index (or under host ingest): the host decoder's batches in file order (hostio.stream_bam), cut where
    the next batch starts with the reads that reach past that point carried over (_windows), decoded a window ahead (_prefetch)"""
    batches = hostio.stream_bam(bam, bc.barcodes, min_mapq=params.min_mapping_quality, batch_bytes=int(window_bytes), filters=filters)
    first = next(batches, None)
    if first is None:
        raise ValueError("%s holds no BAM records" % bam)
    return first.contig_names, _bound_on_arrival(bind, first, _prefetch(_windows(itertools.chain([first], batches), len(first.contig_names))))


def _bound_on_arrival(bind, dec, windows):
    """the windows, dec's contigs bound as the first of them arrives (in the count loop, whose errors the ranks vote on)"""
    for i, w in enumerate(windows):
        if i == 0:
            bind(dec.contig_names, dec.contig_len)
        yield w


def _count_windows(eng, work, names, cts, params, tmp, new_step2, t):
    """The count loop of a region run, no collective inside: per window the load, count and step-1 call, per contig its pieces of the
    tables (regions.piece_path) - of the step-2 table too with new_step2 (row-local step 2, _step2_for).  Returns (the rows rank 0 still
    needs per piece, the kinds of cell of the step-2 rows, the report summed over the windows, windows, the last (lo, hi, DecodedBam))."""
    kept: Dict[tuple, bytes] = {}
    kinds, report, n, last = None, {}, 0, None
    if new_step2 is not None:
        t0 = time.time()
        step2 = new_step2()
        head1 = tsvio.step1_head(cts, "##fileDate=x\n").encode()         # (any date: the head is cut off the step-2 text again)
        cut = len(calling.step2_head(head1))
        t["step2"] = time.time() - t0
    for lo, hi, rec, dec in work:
        for k, v in dec.report.items():
            report[k] = report.get(k, 0) + v
        n, last = n + 1, (lo, hi, dec)
        t0 = time.time()
        if rec is not None:                                # (None: the device ingest loaded the reads already)
            eng.load_reads(rec)
        eng.set_region(lo[0], lo[1], hi[0], hi[1])
        t["load"] += time.time() - t0
        t0 = time.time()
        eng.pileup_count(params.count())
        eng.call_step1(params.call())
        t["gpu_count_call"] += time.time() - t0
        t0 = time.time()
        per_ct = [eng.fetch_counts(ct) for ct in range(len(cts))]
        calls = eng.fetch_calls()
        t["fetch"] += time.time() - t0
        t0 = time.time()
        ckeys = calls["key"] if len(calls) else np.zeros(0, np.int64)
        for tid in np.unique(ckeys >> 32).tolist():
            k_lo, k_hi = tid << 32, (tid + 1) << 32
            sl = [slice(int(np.searchsorted(k, k_lo)), int(np.searchsorted(k, k_hi))) for k, _, _ in per_ct]
            sub = [(k[s_], r[s_], c[s_]) for (k, r, c), s_ in zip(per_ct, sl)]
            c0, c1 = int(np.searchsorted(ckeys, k_lo)), int(np.searchsorted(ckeys, k_hi))
            start1 = int(ckeys[c0] & 0xFFFFFFFF) + 1
            chrom = names[tid]
            for ct, name in enumerate(cts):
                if len(sub[ct][0]):
                    tsvio.write_counts_tsv(regions.piece_path(tmp, chrom, start1, "counts." + name), *sub[ct], names, "", header=False)
            tsvio.write_merged_tsv(regions.piece_path(tmp, chrom, start1, "merged"), sub, names, cts, header=False)
            rows1 = tsvio.write_step1_tsv(regions.piece_path(tmp, chrom, start1, "step1"), calls[c0:c1], sub, names, cts, [], header=False, as_bytes=True)
            if new_step2 is None:
                kept[(chrom, start1)] = rows1
                continue
            t1 = time.time()
            rows2 = step2(head1 + rows1, 0)[cut:] if rows1 else b""
            with open(regions.piece_path(tmp, chrom, start1, "step2"), "wb") as f:
                f.write(rows2)
            if rows2:      # what pandas' dtype inference over the WHOLE step-2 table will see in this piece's rows (calling.step3, all_kinds)
                kinds = _union_kinds(kinds, tsvio.column_kinds(rows2, rows2[:rows2.index(b"\n")].count(b"\t") + 1))
            surv = calling._step3_survivors(rows2, 6) if rows2 and os.environ.get("LONGSOM_STEP3_FULL_PARSE", "0") != "1" else None
            kept[(chrom, start1)] = rows2 if surv is None else surv      # (Cell_types is column 6 of the step-1 / step-2 tables)
            t["step2"] += time.time() - t1
        t["write_tables"] += time.time() - t0
    return kept, kinds, report, n, last


def _union_kinds(a, b):
    """the kinds of cell (tsvio.column_kinds) of two parts of one table, OR-ed; a part with another number of columns starts over"""
    return b.copy() if a is None or len(a) != len(b) else (a | b)


def _assemble(out, tmp, sample_id, cts, report, report_seconds, payloads, kinds, new_step2, params, step3, t):
    """Rank 0's part of a region run: the report; every table as its head and its pieces in (chrom string, start) order; steps 2 and 3
    over the rows that came over the wire - step 2 here only when it did not run where the rows are (new_step2, a distance filter)."""
    t0 = time.time()
    date = tsvio.file_date()
    write_report(out.report, report, report_seconds)
    for name in cts:
        regions.concatenate_pieces(tmp, "counts." + name, tsvio.counts_header("%s.%s" % (sample_id, name), date), out.counts[name])
    regions.concatenate_pieces(tmp, "merged", tsvio.merged_header(cts, date), out.merged)
    head1 = tsvio.step1_head(cts, date)
    regions.concatenate_pieces(tmp, "step1", head1, out.step1)
    t["concatenate"] = time.time() - t0
    t0 = time.time()
    if new_step2 is None:
        # the pieces of the step-2 table are on disk; what came over the wire is the rows step 3 still looks at
        head2 = calling.step2_head(head1.encode())
        regions.concatenate_pieces(tmp, "step2", head2.decode(), out.step2)
        s2 = head2 + regions.unpack_rows_bytes(payloads)
    else:
        s2 = new_step2()(head1.encode() + regions.unpack_rows_bytes(payloads), params.min_distance)
        tsvio.write_bytes(out.step2, s2)
    t["step2"] = t.get("step2", 0.0) + time.time() - t0
    if step3:
        # (s2 holds the survivors of every region when step 2 ran where the rows are: the whole table's dtypes come with `kinds`, the
        # whole table itself - should a foreign cell make its printed form depend on them - from the file just assembled)
        local = {} if new_step2 is not None else {"all_kinds": kinds, "full_text": lambda: open(out.step2, "rb").read()}
        _write_step3(out, s2, params, t, **local)
    shutil.rmtree(tmp, ignore_errors=True)


@dataclass
class ReannoParams:
    """config/config.yaml:40-68 (Reanno block): pass-1 chain parameters + HCCV + re-annotation."""
    # Reanno.BaseCellCalling.  config.yaml:50-51 lists min_ac_cells 5 / min_ac_reads 20, but the reference's pass-1 step-1 rule never
    # forwards them (rules/CellTypeReannotation.smk:208-238) and pass 1 has no step 3, so the script defaults 2 / 3
    # (BaseCellCalling.step1.py:594-595) are what runs; the fused pass 1 does the same
    chain: SnvParams = field(default_factory=SnvParams)
    hccv_min_depth: float = 50
    hccv_delta_vaf: float = 0.2
    hccv_delta_mcf: float = 0.25
    hccv_clust_dist: int = 10000
    chrm_contaminant: str = "False"
    alt_flag: str = "All"
    pvalue: float = 0.01
    genotype_min_bq: int = 30
    min_variants: int = 3
    min_fraction: float = 0.25


@dataclass
class ReannoOutputs:
    pass1: SnvOutputs
    hccv: str
    genotype: str
    barcodes: str
    pass2: Optional[SnvOutputs]
    n_cells_kept: int = 0
    n_cancer: int = 0
    timings: Dict[str, float] = field(default_factory=dict)


def run_reannotation(bam: str, barcodes_tsv: str, ref_fasta: str, out_dir: str, sample_id: str, reanno_params: Optional[ReannoParams] = None,
                     snv_params: Optional[SnvParams] = None, fusions_tsv: Optional[str] = None, editing: Optional[str] = None,
                     pon_sr: Optional[str] = None, pon_lr: Optional[str] = None, gnomad_af_json: Optional[str] = None, device: int = 0,
                     engine: Optional[Engine] = None, pass1_step3: bool = False, comm: Optional["regions.Comm"] = None) -> ReannoOutputs:
    """The two-pass loop of the workflow (rules/CellTypeReannotation.smk + rules/SNVCalling.smk) in one process: the BAM is
    decoded and loaded ONCE; pass 1 calls with the automated annotation, the HCCV sites are genotyped per cell on the resident
    reads, the cells are re-annotated, and pass 2 re-counts the same resident reads under the new barcode table.
    Files: <out>/CellTypeReannotation/{SplitBam,BaseCellCounter,MergeCounts,BaseCellCalling,HCCV,ReannotatedCellTypes}/... and
    <out>/SNVCalling/{SplitBam,BaseCellCounter,MergeCounts,BaseCellCalling}/...
    comm (world > 1, BASELINE config 5 on several GPUs): one rank per GPU, every rank keeps the reads of its region resident across
    both passes (_run_reannotation_ranks)."""
    from . import reanno
    rp = reanno_params or ReannoParams()
    sp = snv_params or SnvParams()
    if comm is not None and comm.world > 1:
        own = engine is None
        eng = engine or Engine(comm.local_device_index)
        try:
            return _run_reannotation_ranks(bam, barcodes_tsv, ref_fasta, out_dir, sample_id, rp, sp, fusions_tsv, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm,
                                           pass1_step3)
        finally:
            if own:
                eng.close()
    own = engine is None
    eng = engine or Engine(device)
    t = {}
    try:
        res = load_sample(bam, barcodes_tsv, ref_fasta, eng, rp.chain.min_mapping_quality, keep_unlisted=True)      # (the genotyping pileup's buffer holds every read)
        d1 = os.path.join(out_dir, "CellTypeReannotation")
        # The HCCV filter runs on the device over the step-2 text while run_chain holds it resident (LONGSOM_HOST_HCCV=1, a step 2 made on
        # the host, or a table the row code leaves undecided: reanno.hccv_filter over the file, as before)
        hccv_args = (rp.hccv_min_depth, rp.hccv_delta_vaf, rp.hccv_delta_mcf, rp.hccv_clust_dist)
        want = None if os.environ.get("LONGSOM_HOST_HCCV", "0") == "1" else HccvRequest(os.path.join(d1, "HCCV", sample_id), *hccv_args)
        p1 = run_chain(res, res.table.celltype_of, res.table.celltype_names, res.dec.report, d1, sample_id, rp.chain, editing, pon_sr, pon_lr, gnomad_af_json,
                       step3=pass1_step3, hccv=want)
        t0 = time.time()
        os.makedirs(os.path.join(d1, "HCCV"), exist_ok=True)
        hccv = p1.hccv or reanno.hccv_filter(p1.step2, os.path.join(d1, "HCCV", sample_id), *hccv_args)
        t["hccv"] = time.time() - t0 + p1.timings.get("hccv_device", 0.0)
        t["hccv_path"] = (p1.hccv_report or {}).get("path", "host") if p1.hccv else "host"      # (which of the two made the files)
        t0 = time.time()
        eng.set_barcodes(res.table.celltype_of, len(res.table.celltype_names))
        geno = os.path.join(d1, "HCCV", sample_id + ".SNVs.SingleCellGenotype.tsv")
        gstats: Dict[str, dict] = {}
        n_rows = reanno.single_cell_genotype(eng, hccv, res.table, res.contig_names, geno, alt_flag=rp.alt_flag, min_bq=rp.genotype_min_bq,
                                             min_mq=rp.chain.min_mapping_quality, alpha2=rp.chain.alpha2, beta2=rp.chain.beta2, pvalue=rp.pvalue,
                                             chrm_contaminant=rp.chrm_contaminant, stats=gstats)
        t["genotype"] = time.time() - t0
        out = ReannoOutputs(p1, hccv, geno, "", None, timings=t)
        if n_rows == 0:                                   # no HCCV: the reference writes no genotype table and the workflow stops here
            return out
        t0 = time.time()
        os.makedirs(os.path.join(d1, "ReannotatedCellTypes"), exist_ok=True)
        out.barcodes = os.path.join(d1, "ReannotatedCellTypes", sample_id + ".tsv")
        out.n_cells_kept, out.n_cancer = reanno.celltype_reannotation(geno, fusions_tsv or "", barcodes_tsv, out.barcodes, rp.min_variants, rp.min_fraction,
                                                                      stats=gstats if os.environ.get("LONGSOM_REANNO_FROM_FILE", "0") != "1" else None)
        t["reannotation"] = time.time() - t0
        # pass 2: same resident reads, new barcode -> cell-type table (cells below coverage are no longer listed)
        if sp.min_mapping_quality != rp.chain.min_mapping_quality:
            raise ValueError("the two passes must share min_mapping_quality to share one decode (SplitBam report)")
        if out.n_cells_kept == 0:
            return out
        ct2, names2 = _pass2_table(out.barcodes, res.table)
        out.pass2 = run_chain(res, ct2, names2, res.dec.report_for(ct2 != 255), os.path.join(out_dir, "SNVCalling"), sample_id, sp, editing,
                              pon_sr, pon_lr, gnomad_af_json)
        return out
    finally:
        if own:
            eng.close()


def _run_reannotation_ranks(bam, barcodes_tsv, ref_fasta, out_dir, sample_id, rp, sp, fusions_tsv, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm,
                            pass1_step3) -> ReannoOutputs:
    """The two-pass loop over several ranks: pass 1 is the sharded SNV run (every rank ingests and keeps its
    region's slice of the BAM, writes its pieces of the tables, rank 0 assembles them); rank 0 filters the HCCVs (a small host step
    over the step-2 table); every rank genotypes the HCCV sites of its own region on its resident reads and the per-(site, barcode)
    tables are summed over the ranks (one all-reduce: sites x barcodes x 2 integers); rank 0 re-annotates the cells; the new barcode ->
    cell-type table reaches the ranks as the file the rule graph writes anyway; pass 2 re-counts the SAME resident reads on every rank.
    No BAM byte is read twice, no read crosses a link: what travels is the candidate rows of both passes and the genotype tables."""
    from . import reanno
    if sp.min_mapping_quality != rp.chain.min_mapping_quality:
        raise ValueError("the two passes must share min_mapping_quality to share one decode (SplitBam report)")
    t: Dict[str, float] = {}
    d1 = os.path.join(out_dir, "CellTypeReannotation")
    eng.set_keep_unlisted(True)                             # (the genotyping pileup's buffer holds every read, listed or not: HCCVSingleCellGenotype.py:121-122)
    old_keep = hostio.set_keep_unlisted(True)
    try:
        p1 = _run_snv_regions(bam, barcodes_tsv, ref_fasta, d1, sample_id, rp.chain, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm, None, step3=pass1_step3)
    finally:
        eng.set_keep_unlisted(False)
        hostio.set_keep_unlisted(old_keep)
    state = p1.resident
    table, dec = state["table"], state["dec"]
    hccv = os.path.join(d1, "HCCV", sample_id + ".HCCV.tsv")
    geno = os.path.join(d1, "HCCV", sample_id + ".SNVs.SingleCellGenotype.tsv")
    t0 = time.time()
    if comm.rank == 0:
        os.makedirs(os.path.join(d1, "HCCV"), exist_ok=True)
        made = reanno.hccv_filter(p1.step2, os.path.join(d1, "HCCV", sample_id), rp.hccv_min_depth, rp.hccv_delta_vaf, rp.hccv_delta_mcf, rp.hccv_clust_dist)
        assert os.path.abspath(made) == os.path.abspath(hccv), (made, hccv)
    comm.barrier()                                          # the HCCV file is there for every rank
    t["hccv"] = time.time() - t0
    t0 = time.time()
    eng.set_barcodes(table.celltype_of, len(table.celltype_names))
    gstats: Dict[str, dict] = {}
    n_rows = reanno.single_cell_genotype(eng, hccv, table, dec.contig_names, geno, alt_flag=rp.alt_flag, min_bq=rp.genotype_min_bq,
                                         min_mq=rp.chain.min_mapping_quality, alpha2=rp.chain.alpha2, beta2=rp.chain.beta2, pvalue=rp.pvalue,
                                         chrm_contaminant=rp.chrm_contaminant, comm=comm, region=(state["lo"], state["hi"]), stats=gstats)
    t["genotype"] = time.time() - t0
    out = ReannoOutputs(p1, hccv, geno, "", None, timings=t)
    if n_rows == 0:
        return out
    t0 = time.time()
    out.barcodes = os.path.join(d1, "ReannotatedCellTypes", sample_id + ".tsv")
    kept = np.zeros(2, np.int64)
    if comm.rank == 0:
        os.makedirs(os.path.join(d1, "ReannotatedCellTypes"), exist_ok=True)
        kept[:] = reanno.celltype_reannotation(geno, fusions_tsv or "", barcodes_tsv, out.barcodes, rp.min_variants, rp.min_fraction,
                                               stats=gstats if os.environ.get("LONGSOM_REANNO_FROM_FILE", "0") != "1" else None)
    kept = comm.allreduce_sum(kept)                          # (also the barrier behind which the new table is on disk)
    out.n_cells_kept, out.n_cancer = int(kept[0]), int(kept[1])
    t["reannotation"] = time.time() - t0
    if out.n_cells_kept == 0:
        return out
    ct2, names2 = _pass2_table(out.barcodes, table)
    out.pass2 = _run_snv_regions(bam, barcodes_tsv, ref_fasta, os.path.join(out_dir, "SNVCalling"), sample_id, sp, editing, pon_sr, pon_lr, gnomad_af_json, eng, comm,
                                 None, resident=state, table=(ct2, names2, dec.report_for(ct2 != 255)))
    return out


def _pass2_table(barcodes_tsv: str, table: "hostio.BarcodeTable"):
    """the re-annotated barcodes.tsv over the barcode ids of the decode (`table`, pass 1's): (cell type per barcode id, 255 = no longer
    listed; the cell-type names)"""
    new = hostio.read_barcodes(barcodes_tsv)
    idx = {b: i for i, b in enumerate(table.barcodes)}
    ct2 = np.full(len(table.barcodes), 255, np.uint8)
    for b, c in zip(new.barcodes, new.celltype_of):
        ct2[idx[b]] = c
    return ct2, new.celltype_names


@dataclass
class PonOutputs:
    pon: str
    step1: Dict[str, str]
    n_sites: int = 0
    timings: Dict[str, Dict[str, float]] = field(default_factory=dict)
    estimates: Optional[List[float]] = None          # fit=True: alpha1, beta1, alpha2, beta2 as fitted from the normals' count rows
    estimates_path: str = ""                         # ... and the BetaBinEstimates.txt they were written to


def pon_params(**kw) -> SnvParams:
    """config/config.yaml:33-37 (PoN block) over the BaseCellCalling step-1 defaults (rules/PoN.smk BaseCellCalling_step1_PoN)."""
    base = dict(min_ac_cells=1, min_ac_reads=1, min_cells=1, min_cell_types=1)
    base.update(kw)
    return SnvParams(**base)


def _pon_fit(eng, normals, ref_fasta, params, comm, n_sites, seed, path) -> List[float]:
    """BetaBinEstimation over the normals' resident count rows: every normal of the rank is loaded and counted (the load makes the
    count and keeps no store), each of its cell types is one table of the fit (csrc/bbfit.hip); the ranks exchange their histograms,
    every rank adds them in rank order and solves - the same integers, so the same bits everywhere - and rank 0 writes the file."""
    cp = params.count()
    first, sample_n = [0] * len(normals), 0
    if n_sites > 0:                                    # the tables' numbers and their count, as every rank must know them: one per (normal, cell type)
        n_ct = [len(hostio.read_barcodes(bct).celltype_names) for _, _, bct in normals]
        first = [sum(n_ct[:i]) for i in range(len(normals))]
        sample_n = bbfit.sample_size(n_sites, sum(n_ct))
    eng.bbfit_reset(bbfit.capacity_for(params.max_depth))          # (no count exceeds the pileup's max_depth)
    for i in range(comm.rank, len(normals), comm.world):
        sample_id, bam, barcodes_tsv = normals[i]
        res = load_sample(bam, barcodes_tsv, ref_fasta, eng, params.min_mapping_quality, count_params=cp, keep_store=False)
        eng.set_barcodes(res.table.celltype_of, len(res.table.celltype_names))
        eng.pileup_count(cp)
        for ct in range(len(res.table.celltype_names)):
            eng.bbfit_accumulate(ct, table=first[i] + ct, sample_n=sample_n, seed=seed)
    if comm.world > 1:
        mine = eng.bbfit_fetch()
        top = int(np.flatnonzero(mine.any(axis=0))[-1]) + 1 if mine.any() else 0          # (the occupied part alone goes over the wire)
        eng.bbfit_reset(mine.shape[1])
        for blob in comm.allgather_bytes(np.ascontiguousarray(mine[:, :top]).tobytes()):
            part = np.frombuffer(blob, np.uint64).reshape(6, -1)
            full = np.zeros_like(mine)
            full[:, :part.shape[1]] = part
            eng.bbfit_add(full)
    est, _ = bbfit.device_solve(eng)
    if comm.rank == 0:
        bbfit.write_estimates(path, est)
    return est


def run_pon(normals, ref_fasta: str, out_dir: str, params: Optional[SnvParams] = None, min_samples: int = 1, rm_prefix: str = "No",
            write_tables: bool = True, out_name: str = "PoN_LR.tsv", device: int = 0, engine: Optional[Engine] = None,
            comm: Optional["regions.Comm"] = None, fit: bool = False, fit_n_sites: int = 0, fit_seed: int = 1992) -> PonOutputs:
    """rules/PoN.smk from SplitBam_PoN to PoN in one process: for every normal (id, bam, barcodes.tsv) the count + step-1 call
    chain, then scripts/PoN/PoN.py over the sites with a filter status.  The beta-binomial parameters come in through `params`
    (BetaBinEstimates.txt's four numbers), or are fitted here (fit=True, below).  write_tables=False skips the per-normal tables (the PoN needs only the call
    records); the PoN file is the same either way.  Output layout: <out_dir>/PoN/{SplitBam,BaseCellCounter,MergeCounts,
    BaseCellCalling,PoN}/ as in the rule file.  comm (world > 1): the normals are independent samples — rank r takes every world-th one
    on its own GPU, the sites of their call records are gathered (one all-gather of a few MB) and rank 0 writes the panel.
    fit=True: the four beta-binomial parameters of `params` are not read; a first pass counts every normal and fits them from the
    resident rows (_pon_fit: BetaBinEstimation.py without R), <out_dir>/PoN/PoN/BetaBinEstimates.txt is written, and the loop runs with
    the fitted values.  fit_n_sites / fit_seed: BetaBinEstimation.py's --n_sites (0, the default here: every eligible site) and --seed."""
    import json
    params = params or pon_params()
    comm = comm or regions.Comm()
    own = engine is None
    eng = engine or Engine(comm.local_device_index if comm.world > 1 else device)
    root = os.path.join(out_dir, "PoN")
    entries, step1, timings = [], {}, {}
    normals = list(normals)
    estimates, estimates_path = None, ""
    try:
        if fit:
            estimates_path = os.path.join(root, "PoN", "BetaBinEstimates.txt")
            estimates = _pon_fit(eng, normals, ref_fasta, params, comm, fit_n_sites, fit_seed, estimates_path)
            params = dataclasses.replace(params, alpha1=estimates[0], beta1=estimates[1], alpha2=estimates[2], beta2=estimates[3])
        for sample_id, bam, barcodes_tsv in normals[comm.rank::comm.world]:
            res = load_sample(bam, barcodes_tsv, ref_fasta, eng, params.min_mapping_quality)
            out, _, calls, t = chain_step1(res, res.table.celltype_of, res.table.celltype_names, res.dec.report, root, sample_id, params, write_tables)
            label = sample_id + ".calling.step1.tsv"          # basename of the table, the sample id of PoN.py:55
            entries += pon.sites_of_calls(calls, res.contig_names, label)
            step1[sample_id] = out.step1
            timings[sample_id] = t
    finally:
        if own:
            eng.close()
    if comm.world > 1:
        # (plain JSON over the wire, the sites' byte fields as latin-1 text: nothing a peer sends is executed on arrival)
        mine = json.dumps({"entries": [[f.decode("latin-1") for f in e] for e in entries], "step1": step1, "timings": timings})
        entries, step1, timings = [], {}, {}
        for blob in comm.allgather_bytes(mine.encode("latin-1")):
            d = json.loads(blob.decode("latin-1"))
            entries += [tuple(f.encode("latin-1") for f in e) for e in d["entries"]]
            step1.update(d["step1"]); timings.update(d["timings"])
    path = os.path.join(root, "PoN", out_name)
    text = pon.pon_text(entries, min_samples, rm_prefix)          # (sorted inside: the panel does not depend on which rank took which normal)
    if comm.rank == 0:
        os.makedirs(os.path.join(root, "PoN"), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    comm.barrier()
    return PonOutputs(path, step1, sum(1 for l in text.split("\n") if l and not l.startswith("#")), timings, estimates, estimates_path)
