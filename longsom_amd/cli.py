"""Command-line entry points with the flag surface of the reference's rule scripts, so that
a rule's `shell:` line keeps working when only its `script=` path changes.  Each function names the
reference CLI it stands in for.  `snv` is the fused entry (one decode, everything resident in HBM)."""
import argparse
import glob
import json
import os
import sys
import time

from . import calling, hostio, pipeline, tsvio
from ._lib import CallParams, CountParams
from .engine import Engine


def _limit(text):
    """--max_nM / --max_NH: an int, or off (None) for an empty value - what a rule renders when its config sets no limit (--max_nM=)"""
    return None if text in ("", "None") else int(text)


def split_bam(argv=None):
    """SplitBamCellTypes.py --bam --meta --id --max_nM --max_NH --min_MQ --n_trim --outdir  (SplitBamCellTypes.py:194-204)"""
    ap = argparse.ArgumentParser(description="Split a BAM into one BAM per cell type by CB tag")
    ap.add_argument("--bam", required=True); ap.add_argument("--meta", required=True); ap.add_argument("--id", default="Sample")
    ap.add_argument("--max_nM", type=_limit, default=None); ap.add_argument("--max_NH", type=_limit, default=None)
    ap.add_argument("--min_MQ", type=int, default=255); ap.add_argument("--n_trim", type=int, default=0); ap.add_argument("--outdir", default=".")
    ap.add_argument("--device", type=int, default=None, help="make the BAMs on this GPU (default: on the host)")
    ap.add_argument("--index", action="store_true", help="also write {id}.{celltype}.bam.bai beside every BAM (pysam.index, SplitBamCellTypes.py:189-192)")
    a = ap.parse_args(argv)
    t0 = time.time()
    table = hostio.read_barcodes(a.meta)
    outs = [os.path.join(a.outdir, "%s.%s.bam" % (a.id, ct)) for ct in table.celltype_names]
    filters = hostio.SplitFilters(a.max_nM, a.max_NH, a.n_trim)
    rep = None
    if a.device is not None:
        rep = _split_bam_device(a.bam, table, outs, a.min_MQ, filters, a.device, a.index)
    if rep is None:
        rep = hostio.split_bam(a.bam, table, outs, a.min_MQ, filters)
        if a.index:
            for path in outs:
                hostio.build_bai(path, full=True)
    pipeline.write_report(os.path.join(a.outdir, a.id + ".report.txt"), rep, time.time() - t0)


def _split_bam_device(bam, table, outs, min_mapq, filters, device, index=False):
    """The cell types' BAMs made on the device (lsg_split_bam) and streamed into their files, one lsg_append_table per cell type on a thread
    of its own; returns the report, or None - said on stderr - for a BAM the host twin has to split: its record chain does not settle
    (rc -4) or it does not fit the device (rc -3)."""
    import threading
    from . import _lib
    try:
        with Engine(device) as eng:
            eng.set_split_filters(filters)
            if index:
                eng.set_split_index(True)
            info = eng.split_bam(bam, table.barcodes, table.celltype_of, len(table.celltype_names), min_mapq)
            errors = []

            def stream(t, path):
                try:
                    open(path, "wb").close()
                    eng.append_table(eng.TABLE_SPLIT_BAM + t, path)
                    if index:                   # (after the BAM: an index older than its file is not used, hostio.find_bai)
                        open(path + ".bai", "wb").close()
                        eng.append_table(eng.TABLE_SPLIT_BAI + t, path + ".bai")
                except Exception as e:      # noqa: BLE001 - handed to the caller's thread below
                    errors.append(e)
            threads = [threading.Thread(target=stream, args=(t, path)) for t, path in enumerate(outs)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            if errors:
                raise errors[0]
            return hostio.split_report(info["counters"], [(info["reasons_n"], info["reasons_first"])])
    except _lib.LsgError as e:
        if e.rc not in (-4, -3):
            raise
        print("%s: %s; splitting it on the host" % (bam, "its records straddle its BGZF blocks" if e.rc == -4 else "it does not fit the device"), file=sys.stderr)
    return None


def index_bam(argv=None):
    """samtools index / pysam.index: --bam X [--out X.bai] [--device N] - the whole .bai (bins, chunks, linear index) of a coordinate-sorted
    BAM in this project's canonical form; rule IndexBam_gpu, the drop-in for IndexBarcodedBam_PoN.  Without --device, and
    for a BAM the device hands back (said on stderr), the host twin writes it."""
    from . import _lib
    ap = argparse.ArgumentParser(description="Index a coordinate-sorted BAM: write its .bai")
    ap.add_argument("--bam", required=True); ap.add_argument("--out", default=None, help="the index file (default: <bam>.bai)")
    ap.add_argument("--device", type=int, default=None, help="make the index on this GPU (default: on the host)")
    a = ap.parse_args(argv)
    t0 = time.time()
    out = a.out or a.bam + ".bai"
    where = "host"
    if a.device is not None:
        try:
            with Engine(a.device) as eng:
                info = eng.bam_index(a.bam)
                open(out, "wb").close()
                eng.append_table(eng.TABLE_BAI, out)
                where = "device"
        except _lib.LsgError as e:
            if e.rc not in (-4, -3):
                raise
            print("%s: %s; indexing it on the host" % (a.bam, "its records straddle its BGZF blocks" if e.rc == -4 else "it does not fit the device"), file=sys.stderr)
    if where == "host":
        hostio.build_bai(a.bam, out, full=True)
        info = {"n_records": None, "n_bytes": os.path.getsize(out)}
    print(json.dumps({"bai": out, "records": info["n_records"], "bytes": info["n_bytes"], "indexed_on": where, "seconds": round(time.time() - t0, 3)}))


def _print_fastq(bam, fastq, table, min_mapq, filters, device, host):
    """BAM -> FASTQ file: printed on the device (lsg_bam_fastq) and streamed into the file with lsg_append_table; `host`, or a BAM whose
    record chain the device cannot settle (rc -4, said on stderr), takes the host twin.  Returns (info dict, "device" | "host")."""
    from . import _lib
    if not host:
        try:
            with Engine(device) as eng:
                if table is not None:
                    eng.set_split_filters(filters)
                info = eng.bam_fastq(bam, None if table is None else table.barcodes, None if table is None else table.celltype_of,
                                     0 if table is None else len(table.celltype_names), min_mapq)
                open(fastq, "wb").close()
                eng.append_table(eng.TABLE_FASTQ, fastq)
                return info, "device"
        except _lib.LsgError as e:
            if e.rc != -4:
                raise
            print("%s: its records straddle its BGZF blocks; printing it on the host" % bam, file=sys.stderr)
    return hostio.bam_fastq(bam, fastq, table, min_mapq, filters), "host"


def bam_to_fastq(argv=None):
    """BamToFastq.py --bam --fastq  (FusionCalling/BamToFastq.py:44-48); --device N / --host are this project's"""
    ap = argparse.ArgumentParser(description="Convert a BAM into the FASTQ ctat-LR-fusion reads: @CB^UMI^name")
    ap.add_argument("--bam", required=True); ap.add_argument("--fastq", required=True)
    ap.add_argument("--device", type=int, default=0); ap.add_argument("--host", action="store_true", help="print on the host (no GPU)")
    a = ap.parse_args(argv)
    t0 = time.time()
    info, where = _print_fastq(a.bam, a.fastq, None, 0, None, a.device, a.host)
    print(json.dumps({"fastq": a.fastq, "records": info["n_printed"][0], "bytes": info["n_bytes"][0], "printed_on": where, "seconds": round(time.time() - t0, 3)}))


def fusion_fastq(argv=None):
    """The unsplit BAM + the barcode table -> {outdir}/{id}.fastq: the reads SplitBamCellTypes writes per cell type, printed cell type after
    cell type - rules BamToFastq + ConcatFastq without the split BAMs (workflow/rules/FusionCalling.gpu.smk FusionFastq_gpu)."""
    ap = argparse.ArgumentParser(description="FASTQ for ctat-LR-fusion from the unsplit BAM, routed by cell type on the GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--meta", required=True); ap.add_argument("--id", default="Sample"); ap.add_argument("--outdir", default=".")
    ap.add_argument("--min_MQ", type=int, default=255)
    ap.add_argument("--max_nM", type=_limit, default=None); ap.add_argument("--max_NH", type=_limit, default=None)
    ap.add_argument("--device", type=int, default=0); ap.add_argument("--host", action="store_true", help="print on the host (no GPU)")
    ap.add_argument("--per_celltype", action="store_true", help="also write {id}.{celltype}.fastq, the files rule BamToFastq made")
    a = ap.parse_args(argv)
    t0 = time.time()
    table = hostio.read_barcodes(a.meta)
    os.makedirs(a.outdir, exist_ok=True)
    out = os.path.join(a.outdir, a.id + ".fastq")
    info, where = _print_fastq(a.bam, out, table, a.min_MQ, hostio.SplitFilters(a.max_nM, a.max_NH, 0), a.device, a.host)
    if a.per_celltype:
        with open(out, "rb") as f:
            for t, ct in enumerate(table.celltype_names):
                with open(os.path.join(a.outdir, "%s.%s.fastq" % (a.id, ct)), "wb") as g:
                    left = info["n_bytes"][t]
                    while left:
                        piece = f.read(min(left, 64 << 20))
                        if not piece:
                            raise RuntimeError("%s is %d bytes shorter than the %d bytes printed for %s" % (out, left, info["n_bytes"][t], ct))
                        g.write(piece); left -= len(piece)
    print(json.dumps({"fastq": out, "records": dict(zip(table.celltype_names, info["n_printed"])), "bytes": dict(zip(table.celltype_names, info["n_bytes"])),
                      "printed_on": where, "seconds": round(time.time() - t0, 3)}))


def _resident_for_gene_counts(eng, bam, table, lens, first, filters):
    """the BAM's reads resident with no load filter (a count under --min_MQ 0 admits every record): the device ingest, the host decoder for
    a BAM whose records straddle its BGZF blocks"""
    from . import _lib
    eng.set_contigs(lens)
    eng.set_barcodes(table.celltype_of, len(table.celltype_names))
    with eng.loading(filters=filters):
        try:
            eng.load_bam(bam, table.barcodes, min_mapq=0, first_record_offset=first)
        except _lib.LsgError as e:
            if e.rc != -4:
                raise
            print("%s: its records straddle its BGZF blocks; decoding it on the host" % bam, file=sys.stderr)
            eng.load_reads(hostio.decode_bam(bam, table.barcodes, min_mapq=0, filters=filters).records)


def gene_counts(argv=None):
    """The unsplit BAM + the barcode table + a GTF -> {outdir}/{id}.counts.formated.txt, the cell-by-gene read counts inferCNV reads, and
    {id}.counts.summary.tsv: rules split_per_bc + featureCount + format_featureCount (workflow/rules/CNACalling.smk:11-75) without the
    per-barcode BAMs (workflow/rules/CNACalling.gpu.smk GeneCounts_gpu; longsom_amd/genecounts.py states what is counted)."""
    ap = argparse.ArgumentParser(description="Cell-by-gene read counts (featureCounts' exon / gene_id / unstranded defaults) of a BAM on the GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--meta", required=True); ap.add_argument("--gtf", required=True)
    ap.add_argument("--names_gtf", default="", help="the GTF whose `gene` lines name the gene ids (default: --gtf)")
    ap.add_argument("--id", default="Sample"); ap.add_argument("--outdir", default=".")
    ap.add_argument("--min_MQ", type=int, default=0, help="featureCounts -Q")
    ap.add_argument("--primary_only", action="store_true", help="featureCounts --primary: secondary and supplementary records are not counted")
    ap.add_argument("--gene_names", default="third", help="third (format_featureCount's rule: the third attribute of a gene line), gene_name, or none (rows are gene ids)")
    ap.add_argument("--tsv", action="store_true", help="tabs instead of commas (infercnv.R reads tabs)")
    ap.add_argument("--max_NH", type=_limit, default=None, help="SplitBamCellTypes' NH limit for BAMs that carry the tag (reads without it are dropped too)")
    ap.add_argument("--device", type=int, default=0); ap.add_argument("--host", action="store_true", help="count on the host (no GPU)")
    a = ap.parse_args(argv)
    from . import genecounts
    if a.gene_names not in genecounts.NAME_RULES:
        ap.error("--gene_names %s: one of %s" % (a.gene_names, ", ".join(genecounts.NAME_RULES)))
    t0 = time.time()
    table = hostio.read_barcodes(a.meta)
    filters = hostio.SplitFilters(None, a.max_NH, 0) if a.max_NH is not None else None
    flag_exclude = genecounts.FLAG_EXCLUDE | (genecounts.FLAG_PRIMARY_ONLY if a.primary_only else 0)
    names, lens, first = hostio.bam_header(a.bam)
    ann = genecounts.load_annotation(a.gtf, names)
    rows, row_of_gene = genecounts.name_rows(ann, a.gtf, a.names_gtf or None, a.gene_names)
    order = genecounts.column_order(table.barcodes)
    sep = "\t" if a.tsv else ","
    os.makedirs(a.outdir, exist_ok=True)
    out = os.path.join(a.outdir, a.id + ".counts.formated.txt")
    if a.host:
        rec = hostio.decode_bam(a.bam, table.barcodes, min_mapq=0, filters=filters).records
        matrix, tallies = genecounts.count(rec, ann, row_of_gene, len(rows), len(table.barcodes), a.min_MQ, flag_exclude)
        text, info = genecounts.matrix_text(matrix, rows, table.barcodes, order, sep), {}
    else:
        with Engine(a.device) as eng:
            _resident_for_gene_counts(eng, a.bam, table, lens, first, filters)
            info, tallies, text = genecounts.device_matrix(eng, ann, rows, row_of_gene, table.barcodes, order, sep, a.min_MQ, flag_exclude, out_path=out)
    _, summary = genecounts.write_outputs(a.outdir, a.id, text, tallies, table.barcodes, order)
    print(json.dumps({"counts": out, "summary": summary, "genes": ann.n_genes, "rows": len(rows), "intervals": ann.n_intervals, "exons_on_absent_contigs": ann.n_dropped_exons,
                      "reads": {k: int(tallies[:, i].sum()) for i, k in enumerate(genecounts.OUTCOMES)}, "counted_on": "host" if a.host else "device",
                      "ms": {k[3:]: round(float(v), 3) for k, v in info.items() if k.startswith("ms_")}, "seconds": round(time.time() - t0, 3)}))


def somatic_fusions(argv=None):
    """FusionCalling.py --fusions --barcodes --min_ac_reads --min_ac_cells --max_MCF_noncancer --deltaMCF --outdir  (FusionCalling.py:88-97)"""
    from . import fusions
    ap = argparse.ArgumentParser(description="Report all fusions found in cancer cells and passing filters")
    ap.add_argument("--fusions", required=True); ap.add_argument("--barcodes", required=True)
    ap.add_argument("--min_ac_reads", type=int, required=True); ap.add_argument("--min_ac_cells", type=int, required=True)
    ap.add_argument("--max_MCF_noncancer", type=float, required=True); ap.add_argument("--deltaMCF", type=float, required=True)
    ap.add_argument("--outdir", required=True)
    a = ap.parse_args(argv)
    fusions.fusion_report(a.fusions, a.barcodes, a.min_ac_reads, a.min_ac_cells, a.max_MCF_noncancer, a.deltaMCF, a.outdir)


def _read_bed(path):
    out = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if len(f) < 3 or line.startswith(("#", "track", "browser")):
            continue
        out.setdefault(f[0], []).append((int(f[1]), int(f[2])))
    return out


def bed_mask(keys, contig_names, contig_len, bed: str, bed_out: str):
    """Which rows (keys = tid << 32 | 0-based position) lie in the regions MakeWindows leaves (BaseCellCounter.py:81-113): the --bed
    intervals merged when at most 1 bp apart (`merge(d=1)`), clipped to [1, contig length) (`intersect` with the (x, 1, len) list: position 0
    of a contig is never visited, with or without a bed), minus the --bed_out intervals (`subtract`); without --bed, whole contigs.
    window_maker then only cuts the regions into pieces.  bedtools' interval arithmetic restated (pybedtools is not in the reference
    tree nor in this image: unpinned, tests/test_cli_cpu.py holds hand-derived cases)."""
    import numpy as np
    keys = np.asarray(keys, np.int64)
    keep = np.zeros(len(keys), bool)
    want = _read_bed(bed) if bed else None
    drop = _read_bed(bed_out) if bed_out else {}
    tid_of, pos = keys >> 32, keys & 0xFFFFFFFF
    for tid, (name, length) in enumerate(zip(contig_names, contig_len)):
        if want is None:
            ivs = [(1, int(length))]
        else:
            merged = []
            for s0, e0 in sorted(want.get(name, [])):
                if merged and s0 - merged[-1][1] <= 1:
                    merged[-1][1] = max(merged[-1][1], e0)
                else:
                    merged.append([s0, e0])
            ivs = [(max(s0, 1), min(e0, int(length))) for s0, e0 in merged if min(e0, int(length)) > max(s0, 1)]
        sel = np.nonzero(tid_of == tid)[0]
        if not len(sel) or not ivs:
            continue
        p = pos[sel]
        starts = np.asarray([x for x, _ in ivs], np.int64); ends = np.asarray([y for _, y in ivs], np.int64)
        j = np.searchsorted(starts, p, side="right") - 1
        inside = (j >= 0) & (p < ends[np.maximum(j, 0)])
        for s0, e0 in drop.get(name, []):
            inside &= ~((p >= s0) & (p < e0))
        keep[sel] = inside
    return keep


def base_cell_counter(argv=None):
    """BaseCellCounter.py --bam --ref --chrom --out_folder --nprocs --min_mq --tmp_dir [...]  (BaseCellCounter.py:323-342).
    --bam is one cell type's BAM: every CB in it is a cell of that type."""
    ap = argparse.ArgumentParser(description="Per-cell-type pileup base counting on the GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--ref", required=True); ap.add_argument("--chrom", required=True)
    ap.add_argument("--out_folder", default="."); ap.add_argument("--id"); ap.add_argument("--nprocs", type=int, default=1)
    ap.add_argument("--bin", type=int, default=50000); ap.add_argument("--bed", default=""); ap.add_argument("--bed_out", default="")
    ap.add_argument("--min_ac", type=int, default=0); ap.add_argument("--min_af", type=float, default=0); ap.add_argument("--min_dp", type=int, default=5)
    ap.add_argument("--min_cc", type=int, default=5); ap.add_argument("--min_bq", type=int, default=20); ap.add_argument("--min_mq", type=int, default=255)
    ap.add_argument("--tmp_dir", default="."); ap.add_argument("--device", type=int, default=0)
    _add_htslib_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a)
    if a.min_ac:
        raise SystemExit("--min_ac counts alternative alleles over every read of the pileup column, supplementary ones included (BaseCellCounter.py:152-180,221); "
                         "LongSom's rules never pass it and it is not implemented")
    sid = a.id or os.path.basename(a.bam).replace(".bam", "")
    if a.tmp_dir != ".":
        os.makedirs(a.tmp_dir, exist_ok=True)          # the rule declares it as an output (R:SNVCalling.smk:36)
    dec = hostio.decode_bam(a.bam, None, min_mapq=a.min_mq)
    names, seqs = tsvio.read_fasta(a.ref)
    seq_of = dict(zip(names, seqs))
    with Engine(a.device) as eng:
        eng.set_contigs(dec.contig_len)
        for tid, n in enumerate(dec.contig_names):
            eng.load_reference(tid, seq_of[n])
        import numpy as np
        eng.set_barcodes(np.zeros(max(1, len(dec.barcodes)), np.uint8), 1)
        if a.chrom != "all":
            tid = dec.contig_names.index(a.chrom)
            eng.set_region(tid, 0, tid + 1, 0)
        eng.set_pileup_window(max(64, a.bin))             # --bin: the windows whose pileups each have a max_depth buffer of their own (:185-191)
        cp = CountParams.longsom_defaults(min_bq=a.min_bq, min_mq=a.min_mq, min_dp=a.min_dp, min_cc=a.min_cc)
        eng.set_count_at_load(cp)                         # this script counts its BAM once: in the pass that loads it,
        eng.set_store_policy(eng.STORE_SKIP_WHEN_COUNTED)  # and keeps no store for another count
        eng.set_load_filter(cp.min_mq, cp.flag_exclude, cp.ignore_orphans)      # (reads the count would refuse are not stored: keys alone through the sort)
        eng.load_reads(dec.records)
        eng.pileup_count(cp)
        out = os.path.join(a.out_folder, sid + ".tsv")
        print("Outfile: ", out, "\n")
        if not (a.bed or a.bed_out) and os.environ.get("LONGSOM_HOST_TABLES", "0") != "1":
            # the table is printed where its rows lie and streamed into the file (csrc/tables.hip; the same bytes as the writer below)
            eng.set_table_names(dec.contig_names, [sid])
            eng.format_table(eng.TABLE_COUNTS)
            with open(out, "w") as f:
                f.write(tsvio.counts_header(sid))
            eng.append_table(eng.TABLE_COUNTS, out)
            return
        k, r, c = eng.fetch_counts(0)
    if a.bed or a.bed_out:                                # MakeWindows' interval arithmetic (BaseCellCounter.py:88-106): only rows inside are written
        keep = bed_mask(k, dec.contig_names, [len(seq_of[n]) for n in dec.contig_names], a.bed, a.bed_out)
        k, r, c = k[keep], r[keep], c[keep]
    tsvio.write_counts_tsv(out, k, r, c, dec.contig_names, sid)


def merge_counts(argv=None):
    """MergeBaseCellCounts.py --tsv_folder --outfile  (MergeBaseCellCounts.py:206-210); columns in sorted file order."""
    ap = argparse.ArgumentParser(description="Merge per-cell-type base count TSVs")
    ap.add_argument("--tsv_folder", required=True); ap.add_argument("--outfile", required=True)
    a = ap.parse_args(argv)
    files = sorted(glob.glob(a.tsv_folder + "/*.tsv"))
    if not files:
        raise RuntimeError("No tsv files found")
    contigs = tsvio.contigs_of_tsv(files)
    per_ct = [tsvio.parse_counts_tsv(f, contigs)[:3] for f in files]
    cts = [os.path.basename(f).split(".")[-2] for f in files]
    tsvio.write_merged_tsv(a.outfile, per_ct, contigs, cts)


def calling_step1(argv=None):
    """BaseCellCalling.step1.py --infile --outfile --ref --min_cell_types --min_ac_reads --min_ac_cells --alpha1 ...  (step1.py:585-604)"""
    ap = argparse.ArgumentParser(description="Beta-binomial somatic test on the GPU")
    ap.add_argument("--infile", required=True); ap.add_argument("--outfile", required=True); ap.add_argument("--ref", required=True)
    ap.add_argument("--editing"); ap.add_argument("--pon")
    ap.add_argument("--min_cov", type=int, default=5); ap.add_argument("--min_cells", type=int, default=5)
    ap.add_argument("--min_ac_cells", type=int, default=2); ap.add_argument("--min_ac_reads", type=int, default=3)
    ap.add_argument("--max_cell_types", type=int, default=1); ap.add_argument("--min_cell_types", type=int, default=2)
    ap.add_argument("--fisher_cutoff", type=float, default=1); ap.add_argument("--min_distance", type=int, default=5)
    ap.add_argument("--alpha1", type=float, default=0.21356677091082193); ap.add_argument("--beta1", type=float, default=104.95163748636298)
    ap.add_argument("--alpha2", type=float, default=0.2474528917555431); ap.add_argument("--beta2", type=float, default=162.03696139428595)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.fisher_cutoff != 1:
        raise SystemExit("--fisher_cutoff other than 1 (strand test off) is not implemented")
    names, seqs = tsvio.read_fasta(a.ref)
    cts, per_ct, header = tsvio.parse_merged_tsv(a.infile, names)
    with Engine(a.device) as eng:
        eng.set_contigs([len(s) for s in seqs])
        for t, s in enumerate(seqs):
            eng.load_reference(t, s)
        eng.load_counts([p[0] for p in per_ct], [p[2] for p in per_ct])
        eng.call_step1(CallParams.longsom_defaults(alpha1=a.alpha1, beta1=a.beta1, alpha2=a.alpha2, beta2=a.beta2, min_cov=a.min_cov,
                                                   min_cells=a.min_cells, min_ac_cells=a.min_ac_cells, min_ac_reads=a.min_ac_reads,
                                                   max_cell_types=a.max_cell_types, min_cell_types=a.min_cell_types))
        if os.environ.get("LONGSOM_HOST_TABLES", "0") != "1" and not any(ch in n for n in list(names) + list(cts) for ch in "\t\n"):
            eng.set_table_names(names, cts)
            eng.format_table(eng.TABLE_STEP1)
            with open(a.outfile + ".calling.step1.tsv", "w") as f:
                f.write(tsvio.step1_header(header, cts))
            eng.append_table(eng.TABLE_STEP1, a.outfile + ".calling.step1.tsv")
            return
        calls = eng.fetch_calls()
    tsvio.write_step1_tsv(a.outfile + ".calling.step1.tsv", calls, per_ct, names, cts, header)


def calling_step2(argv=None):
    """BaseCellCalling.step2.py --infile --outfile --editing --pon_SR --pon_LR --gnomAD_db --gnomAD_max --min_distance  (step2.py:237-248).
    --gnomAD_db: the gnomad_db directory the reference's rule passes (read with sqlite3) or a JSON {"chrom:pos:ref:alt": AF};
    a source that cannot be used switches the filter off WITH a warning on stderr."""
    ap = argparse.ArgumentParser(description="Position-set / distance / gnomAD tags")
    ap.add_argument("--infile", required=True); ap.add_argument("--outfile", required=True); ap.add_argument("--editing")
    ap.add_argument("--pon_SR", required=True); ap.add_argument("--pon_LR", nargs="?", const="", default="")
    ap.add_argument("--min_distance", type=int, default=5); ap.add_argument("--gnomAD_db"); ap.add_argument("--gnomAD_max", type=float, default=0.01)
    ap.add_argument("--reference-gz-compat", action="store_true"); ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--allow_missing_gnomad", action="store_true", help="run without the gnomAD filter when --gnomAD_db cannot be read (default: stop, as the reference does)")
    a = ap.parse_args(argv)
    text = open(a.infile, "rb").read()
    contigs = tsvio.contigs_of_tsv([a.infile])
    af = calling.open_gnomad(a.gnomAD_db, a.allow_missing_gnomad or None)               # JSON table, gnomad_db directory / sqlite
    keys = [calling.read_posset_keys(p, contigs, a.reference_gz_compat) for p in (a.editing, a.pon_SR, a.pon_LR)]
    with Engine(a.device) as eng:
        out = calling.step2_bytes(text, eng, contigs, keys[0], keys[1], keys[2], a.min_distance, af, a.gnomAD_max)
    with open(a.outfile + ".calling.step2.tsv", "wb") as f:
        f.write(out)


def calling_step3(argv=None):
    """BaseCellCalling.step3.py --infile --outfile --deltaVAF --deltaMCF --chrM_contaminant --min_ac_reads --min_ac_cells --clust_dist  (step3.py:318-328).
    Flags of this script alone: --device N decides and prints the rows on GPU N (the table is uploaded), --native with the host twin of the
    same row code; a table the row code does not decide runs through calling.step3, as every table does without either flag."""
    ap = argparse.ArgumentParser(description="LongSom final filters")
    ap.add_argument("--infile", required=True); ap.add_argument("--outfile", required=True)
    ap.add_argument("--deltaVAF", type=float, required=True); ap.add_argument("--deltaMCF", type=float, required=True)
    ap.add_argument("--chrM_contaminant", default="True"); ap.add_argument("--min_ac_reads", type=int, default=2)
    ap.add_argument("--min_ac_cells", type=int, default=3); ap.add_argument("--clust_dist", type=int, default=5)
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--device", type=int, default=None); how.add_argument("--native", action="store_true")
    a = ap.parse_args(argv)
    if a.device is not None or a.native:
        args = (a.infile, a.outfile + ".calling.step3.tsv", a.outfile + ".calling.step3.unfiltered.tsv", a.deltaVAF, a.deltaMCF, a.min_ac_reads, a.min_ac_cells, a.clust_dist)
        if a.native:
            calling.step3_native(*args)
        else:
            with Engine(a.device) as eng:
                calling.step3_device(eng, *args)
        return
    final, unfiltered = calling.step3(open(a.infile, "rb").read(), a.deltaVAF, a.deltaMCF, a.min_ac_reads, a.min_ac_cells, a.clust_dist)
    open(a.outfile + ".calling.step3.tsv", "w").write(final)
    open(a.outfile + ".calling.step3.unfiltered.tsv", "w").write(unfiltered)


def hccv(argv=None):
    """HighConfidenceCancerVariants.py --SNVs --outfile PREFIX --min_dp --deltaVAF --deltaMCF [--clust_dist]  (:259-267).
    Flags of this script alone: --device N decides and prints the rows on GPU N (the table is uploaded), --native with the host twin of the
    same row code; without either the pandas form runs, as before.  A table the row code does not decide runs through the pandas form."""
    from . import reanno
    ap = argparse.ArgumentParser(description="High-confidence cancer variants for the cell-type re-annotation")
    ap.add_argument("--SNVs", required=True); ap.add_argument("--outfile", required=True)
    ap.add_argument("--min_dp", type=float, required=True); ap.add_argument("--deltaVAF", type=float, required=True)
    ap.add_argument("--deltaMCF", type=float, required=True); ap.add_argument("--clust_dist", type=int, default=10000)
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--device", type=int, default=None); how.add_argument("--native", action="store_true")
    a = ap.parse_args(argv)
    print("\n- High Confidence Cancer Variants calling\n")
    args = (a.SNVs, a.outfile, a.min_dp, a.deltaVAF, a.deltaMCF, a.clust_dist)
    if a.device is not None:
        from .engine import Engine
        with Engine(a.device) as eng:
            reanno.hccv_filter_device(eng, *args)
    elif a.native:
        reanno.hccv_filter_native(*args)
    else:
        reanno.hccv_filter(*args)


def single_cell_genotype(argv=None):
    """HCCVSingleCellGenotype.py --bam --infile --ref --meta --outfile [--alt_flag --nprocs --bin --min_bq --min_mq --tissue
    --tmp_dir --alpha2 --beta2 --pvalue --chrM_contaminant]  (:317-337).  --ref is accepted and not needed (the reference only
    uses it for a count it never reads, :138-145)."""
    from . import reanno
    ap = argparse.ArgumentParser(description="Alleles observed in every cell at the variant sites, on the GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--infile", required=True); ap.add_argument("--ref", required=True)
    ap.add_argument("--meta", required=True); ap.add_argument("--outfile", default="Matrix.tsv")
    ap.add_argument("--alt_flag", default="All", choices=["Alt", "All"]); ap.add_argument("--nprocs", type=int, default=1)
    ap.add_argument("--bin", type=int, default=50000); ap.add_argument("--min_bq", type=int, default=30); ap.add_argument("--min_mq", type=int, default=255)
    ap.add_argument("--tissue", default=None); ap.add_argument("--tmp_dir", default="tmpDir")
    ap.add_argument("--alpha2", type=float, default=0.260288007167716); ap.add_argument("--beta2", type=float, default=173.94711910763732)
    ap.add_argument("--pvalue", type=float, default=0.01); ap.add_argument("--chrM_contaminant", default="True")
    ap.add_argument("--device", type=int, default=0)
    _add_htslib_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a)
    if a.tissue is not None:
        raise SystemExit("--tissue is not used by LongSom's rules and is not implemented")
    print("Outfile: ", a.outfile, "\n")
    os.makedirs(a.tmp_dir, exist_ok=True)              # the rule declares it as an output (R:CellTypeReannotation.smk:316)
    table = hostio.read_barcodes(a.meta)
    dec = hostio.decode_bam(a.bam, table.barcodes, min_mapq=0)
    with Engine(a.device) as eng:
        eng.set_contigs(dec.contig_len)
        eng.set_barcodes(table.celltype_of, len(table.celltype_names))
        eng.load_reads(dec.records)
        reanno.single_cell_genotype(eng, a.infile, table, dec.contig_names, a.outfile, alt_flag=a.alt_flag, window=a.bin, min_bq=a.min_bq,
                                    min_mq=a.min_mq, alpha2=a.alpha2, beta2=a.beta2, pvalue=a.pvalue, chrm_contaminant=a.chrM_contaminant)


def cell_genotype_matrices(argv=None):
    """SingleCellGenotype.py --bam --infile --ref --meta --fusions [FILE] --outfile PREFIX [--alt_flag --nprocs --bin --min_bq --min_mq --tissue
    --tmp_dir --alpha2 --beta2 --pvalue --chrM_contaminant]  (scripts/CellClustering/SingleCellGenotype.py:381-400).  Writes
    PREFIX.SingleCellGenotype.tsv and PREFIX.{Dp,Alt,VAF,Binary}Matrix.tsv.  --ref is accepted and not needed (:127,140).
    With --bnpc_outfile PREFIX2 [--min_cells_per_mut --min_pos_cov --bnpc_barcodes FILE (default: --meta)] the process also writes rule
    FormatInputBnpC's three files from the cells while they are resident (cellclust.format_bnpc_input)."""
    from . import cellclust
    ap = argparse.ArgumentParser(description="SNVs / fusions observed in every cell and the cell-by-variant matrices, on the GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--infile", required=True); ap.add_argument("--ref", required=True)
    ap.add_argument("--meta", required=True); ap.add_argument("--fusions", nargs="?", const="", required=True); ap.add_argument("--outfile", default="Matrix.tsv")
    ap.add_argument("--alt_flag", default="All", choices=["Alt", "All"]); ap.add_argument("--nprocs", type=int, default=1)
    ap.add_argument("--bin", type=int, default=50000); ap.add_argument("--min_bq", type=int, default=30); ap.add_argument("--min_mq", type=int, default=255)
    ap.add_argument("--tissue", default=None); ap.add_argument("--tmp_dir", default="tmpDir")
    ap.add_argument("--alpha2", type=float, default=0.2474528917555431); ap.add_argument("--beta2", type=float, default=162.03696139428595)
    ap.add_argument("--pvalue", type=float, default=0.01); ap.add_argument("--chrM_contaminant", default="True")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--bnpc_outfile", nargs="?", const="", default=""); ap.add_argument("--bnpc_barcodes", default=None)
    ap.add_argument("--min_cells_per_mut", type=int, default=5); ap.add_argument("--min_pos_cov", type=int, default=3)
    _add_htslib_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a)
    if a.tissue is not None:
        raise SystemExit("--tissue is not used by LongSom's rules and is not implemented")
    print("Outfile prefix: ", a.outfile, "\n")
    os.makedirs(a.tmp_dir, exist_ok=True)              # the rule declares it as an output (R:CellClustering.smk:18)
    table = hostio.read_barcodes(a.meta)
    dec = hostio.decode_bam(a.bam, table.barcodes, min_mapq=0)
    with Engine(a.device) as eng:
        eng.set_contigs(dec.contig_len)
        eng.set_barcodes(table.celltype_of, len(table.celltype_names))
        eng.load_reads(dec.records)
        try:
            cellclust.cell_genotype_matrices(eng, a.infile, table, dec.contig_names, a.outfile, a.fusions or None, alt_flag=a.alt_flag, window=a.bin,
                                             min_bq=a.min_bq, min_mq=a.min_mq, alpha2=a.alpha2, beta2=a.beta2, pvalue=a.pvalue, chrm_contaminant=a.chrM_contaminant,
                                             bnpc_prefix=a.bnpc_outfile, bnpc_barcodes=a.bnpc_barcodes or a.meta, min_cells_per_mut=a.min_cells_per_mut,
                                             min_pos_cov=a.min_pos_cov)
        except cellclust.NoTargets as e:
            raise SystemExit(str(e))


def format_input_bnpc(argv=None):
    """FormatInputBnpC.py --bin --vaf --barcodes [--min_cells_per_mut 5 --min_pos_cov 3 --outfile PREFIX]
    (scripts/CellClustering/FormatInputBnpC.py:37-45).  Writes PREFIX.BinaryMatrix.tsv, PREFIX.VAFMatrix.tsv and PREFIX.Barcodes.tsv."""
    from . import cellclust
    ap = argparse.ArgumentParser(description="Filter the cell-by-variant matrices into BnpC's input, on the GPU")
    ap.add_argument("--bin", required=True); ap.add_argument("--vaf", required=True); ap.add_argument("--barcodes", required=True)
    ap.add_argument("--min_cells_per_mut", type=int, default=5); ap.add_argument("--min_pos_cov", type=int, default=3)
    ap.add_argument("--outfile", default="Matrix.tsv"); ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    print("Outfile prefix: ", a.outfile, "\n")
    if os.path.dirname(a.outfile):
        os.makedirs(os.path.dirname(a.outfile), exist_ok=True)
    with Engine(a.device) as eng:
        cellclust.format_bnpc_input_files(eng, a.bin, a.vaf, a.barcodes, a.outfile, a.min_cells_per_mut, a.min_pos_cov)


def _bnpc_parser():
    """the flags of scripts/CellClustering/run_BnpC.py:13-205, and three of this script's own"""
    def ratio(lo_open, hi_open, lo=0.0, hi=1.0):
        def check(val):
            val = float(val)
            if (val <= lo if lo_open else val < lo) or (val >= hi if hi_open else val > hi):
                raise argparse.ArgumentTypeError("Invalid value: %s. Values need to be %s %s x %s %s" % (val, lo, "<" if lo_open else "<=", "<" if hi_open else "<=", hi))
            return val
        return check
    check_ratio, check_percent, check_psrf = ratio(True, True), ratio(False, False), ratio(False, False, 1.0, 1.5)
    ap = argparse.ArgumentParser(prog="BnpC", usage="python3 run_BnpC.py <DATA> [options]",
                                 description="BnpC clustering: the reference's sampler, the posterior estimate on the GPU")
    ap.add_argument("--version", action="version", version="0.2.1")
    ap.add_argument("input", nargs="?", help="the cells' matrix: BnpC_input/<id>.BinaryMatrix.tsv (required)")
    ap.add_argument("-t", "--transpose", action="store_false")
    ap.add_argument("--debug", action="store_true", default=False)
    ap.add_argument("--barcodes", type=str)
    ap.add_argument("--mut_order", type=str, nargs="?", const="", default="")
    m = ap.add_argument_group("model")
    m.add_argument("-FN", "--falseNegative", type=float, default=-1)
    m.add_argument("-FP", "--falsePositive", type=float, default=-1)
    m.add_argument("-FN_m", "--falseNegative_mean", type=check_ratio, default=0.2)
    m.add_argument("-FN_sd", "--falseNegative_std", type=check_ratio, default=0.1)
    m.add_argument("-FP_m", "--falsePositive_mean", type=check_ratio, default=0.01)
    m.add_argument("-FP_sd", "--falsePositive_std", type=check_ratio, default=0.01)
    m.add_argument("-ap", "--DPa_prior", type=float, nargs=2, default=[-1, -1])
    m.add_argument("-pp", "--param_prior", type=float, nargs=2, default=[.25, .25])
    m.add_argument("-fa", "--fixed_assignment", type=str, default="")
    c = ap.add_argument_group("MCMC")
    c.add_argument("-n", "--chains", type=int, default=1)
    c.add_argument("-s", "--steps", type=int, default=5000)
    c.add_argument("-r", "--runtime", type=int, default=-1)
    c.add_argument("-ls", "--lugsail", type=check_psrf, default=-1)
    c.add_argument("-b", "--burn_in", type=check_percent, default=0.33)
    c.add_argument("-cup", "--conc_update_prob", type=check_percent, default=0.25)
    c.add_argument("-eup", "--error_update_prob", type=check_percent, default=0.25)
    c.add_argument("-smp", "--split_merge_prob", type=check_percent, default=0.33)
    c.add_argument("-sms", "--split_merge_steps", type=int, default=3)
    c.add_argument("-smr", "--split_merge_ratios", type=check_percent, nargs=2, default=[0.75, 0.25])
    c.add_argument("-e", "--estimator", type=str, default="posterior", nargs="+", choices=["posterior", "ML", "MAP"])
    c.add_argument("-sc", "--single_chains", action="store_true", default=False)
    c.add_argument("--seed", type=int, default=-1)
    o = ap.add_argument_group("output")
    o.add_argument("-o", "--output", type=str, default="")
    o.add_argument("-v", "--verbosity", type=int, default=1, choices=[0, 1, 2])
    o.add_argument("-np", "--no_plots", action="store_true", default=False)
    o.add_argument("-tr", "--tree", type=str, default="")
    o.add_argument("-tc", "--true_clusters", type=str, default="")
    o.add_argument("-td", "--true_data", type=str, default="")
    g = ap.add_argument_group("this script's own")
    g.add_argument("--bnpc_libs", default="", help="the vendored BnpC's libs/ directory (default: ../../scripts/CellClustering/libs of the checkout this script lies in)")
    g.add_argument("--save_chains", default="", help="write the chains to this .npz")
    g.add_argument("--chains_npz", default="", help="estimate from chains saved by --save_chains: no sampler is run")
    g.add_argument("--host_estimate", action="store_true", help="the numpy twin of the estimate, for a machine without a GPU")
    g.add_argument("--device", type=int, default=0)
    g.add_argument("--scipy_linkage", action="store_true", help="the estimate's ward tree and its cuts by scipy on the host instead of the GPU (the same bits)")
    g.add_argument("--sampler", choices=["reference", "device", "device-sm", "device-errors", "device-open"], default="reference",
                   help="device: Gibbs sweeps, the concentration update and the parameter moves on the GPU, all chains at once (needs -smp 0); "
                        "device-sm: the same with the split-merge move, -smp / -sms / -smr honoured (-smp 0 equals device); "
                        "device-errors: device-sm with the error rates learned (-eup, unless -FP and -FN are both given) and -fa honoured; "
                        "device-open: device-errors with chains of open length: -ls runs until the PSRF is at most the cutoff, -r for a time (-r wins over -ls, both over -s)")
    return ap


def _device_sampler_refusals(a):
    """what longsom_amd.bnpc_sampler does not do, or a --sampler value does not ask of it, each named by its flag; --sampler device and
    device-sm share all but the first, device-errors has only the last two, device-open none of them (and -ls 1 of its own)"""
    like_errors = a.sampler in ("device-errors", "device-open")
    if a.sampler == "device" and a.split_merge_prob != 0:
        sys.exit("run_BnpC.py: --sampler device has no split-merge move: -smp/--split_merge_prob %g is not supported, run it with -smp 0" % a.split_merge_prob)
    who = "--sampler %s" % a.sampler
    if not like_errors and not (a.falsePositive > 0 and a.falseNegative > 0) and a.error_update_prob != 0:
        sys.exit("run_BnpC.py: %s keeps the error rates fixed: -eup/--error_update_prob %g is not supported, run it with -eup 0 (or give -FP and -FN)"
                 % (who, a.error_update_prob))
    if not like_errors and a.fixed_assignment:
        sys.exit("run_BnpC.py: %s does not support -fa/--fixed_assignment" % who)
    if a.sampler == "device-open":
        if not a.runtime > 0 and a.lugsail == 1:
            sys.exit("run_BnpC.py: -ls/--lugsail 1 is not supported: the first run has int(1 / (cutoff^2 - 1)) steps, give a cutoff above 1")
        return
    if a.runtime > 0:
        sys.exit("run_BnpC.py: %s does not support -r/--runtime: give the steps with -s, or run --sampler device-open" % who)
    if a.lugsail > 0:
        sys.exit("run_BnpC.py: %s does not support -ls/--lugsail: give the steps with -s, or run --sampler device-open" % who)


def _device_stop_rule(a, clock=None):
    """--sampler device-open's stop rule from -r, -ls and -s as dpmmIO._get_mcmc_termination (dpmmIO.py:158-169) reads them: -r wins over
    -ls, both over -s.  Returns (the rule: None for -s's steps, what the run is printed as).  a.time[0] is the run's start."""
    from datetime import datetime, timedelta
    from . import bnpc_sampler
    if a.sampler != "device-open" or not (a.runtime > 0 or a.lugsail > 0):
        return None, f"for {a.steps} steps"
    if a.runtime > 0:
        whole = timedelta(minutes=a.runtime)
        return bnpc_sampler.Runtime(a.time[0] + whole, a.time[0] + a.burn_in * whole, clock or datetime.now), f"for {a.runtime} mins"
    report = (lambda steps_run, psrf: print(f"\tPSRF at {steps_run}:\t{psrf:.5f}")) if a.verbosity > 1 else None
    return bnpc_sampler.Lugsail(a.lugsail, report=report), f"until PSRF < {a.lugsail:.4f}"


def _device_chains(a, data):
    """the chains of --sampler device / device-sm / device-errors / device-open: the model of run_BnpC.py:261-296, the seeds drawn as MCMC.run draws them.
    device and device-sm keep the error rates fixed (the given ones, or the priors' means with the priors' own terms in MAP); device-errors
    learns them with -eup unless both are given (run_BnpC.py:261-262), and starts from -fa's labels and keeps them where it is given;
    device-open is device-errors under _device_stop_rule."""
    from scipy.stats import truncnorm
    from . import bnpc_sampler
    learn = {}
    like_errors = a.sampler in ("device-errors", "device-open")
    if a.falsePositive > 0 and a.falseNegative > 0:
        if like_errors:
            a.error_update_prob = 0
        FN, FP, error_prior = a.falseNegative, a.falsePositive, None
    else:
        FN, FP = a.falseNegative_mean, a.falsePositive_mean
        error_prior = sum(float(truncnorm((0 - m) / sd, (1 - m) / sd, m, sd).logpdf(m)) for m, sd in ((FP, a.falsePositive_std), (FN, a.falseNegative_std)))
        if like_errors and a.error_update_prob > 0:
            learn = dict(error_prob=a.error_update_prob, error_priors=(FP, a.falsePositive_std, FN, a.falseNegative_std))
    if like_errors and a.fixed_assignment:
        learn["fixed_assignment"] = bnpc_sampler.load_assignment(a.fixed_assignment)
        if len(learn["fixed_assignment"]) != data.shape[0]:
            sys.exit("run_BnpC.py: -fa/--fixed_assignment %s has %d labels, the data have %d cells" % (a.fixed_assignment, len(learn["fixed_assignment"]), data.shape[0]))
    a.chain_seeds = bnpc_sampler.chain_seeds(a.seed, a.chains)
    stop, run_str = _device_stop_rule(a)
    if a.verbosity > 0:
        print(f"Run MCMC on the device ({a.chains} chains {run_str}, FN {FN} FP {FP}{', learned' if 'error_prob' in learn else ''}):")
    with Engine(a.device) as eng:
        return bnpc_sampler.run_chains(eng, data, [int(s) for s in a.chain_seeds], a.steps, int(a.steps * a.burn_in), FN, FP, pp=a.param_prior, dpa=a.DPa_prior,
                                       dpa_prob=a.conc_update_prob, error_prior=error_prior, sm_prob=a.split_merge_prob if a.sampler != "device" else 0.0,
                                       sm_ratios=tuple(a.split_merge_ratios), sm_steps=a.split_merge_steps, stop=stop, **learn)


def run_bnpc(argv=None):
    """run_BnpC.py: the chains come from the vendored BnpC's sampler (libs/MCMC.py, run as the reference runs it), from --sampler device
    / device-sm / device-errors / device-open (longsom_amd.bnpc_sampler: device-sm with the split-merge move, device-errors also with learned
    error rates and -fa, device-open also with -ls and -r) or from --chains_npz; the
    posterior estimate is made on the device (longsom_amd.bnpc); assignment.txt, errors.txt and genotypes_*.tsv are written here; args.txt,
    the PSRF, -e ML|MAP, the summaries and the plots are left to the checkout's own functions."""
    from datetime import datetime
    from . import bnpc
    ap = _bnpc_parser()
    a = ap.parse_args(argv)
    if a.input is None:
        ap.error("the following arguments are required: input")
    script_dir = os.path.dirname(os.path.abspath(sys.argv[0]))          # the shim's place in the checkout it was dropped into
    if isinstance(a.estimator, str):
        a.estimator = [a.estimator]
    if a.single_chains:
        sys.exit("run_BnpC.py: -sc/--single_chains is not supported here: the posterior estimate is made once, over all chains")
    on_device = a.sampler in ("device", "device-sm", "device-errors", "device-open")
    if on_device and not a.chains_npz:
        _device_sampler_refusals(a)
    point = [e for e in a.estimator if e != "posterior"]
    if a.chains_npz and point:
        sys.exit("run_BnpC.py: -e %s needs the sampler's run: it cannot be combined with --chains_npz" % " ".join(point))
    libs_dir = a.bnpc_libs or os.path.join(script_dir, "..", "..", "scripts", "CellClustering", "libs")
    have_libs = os.path.isfile(os.path.join(libs_dir, "MCMC.py"))
    own_chains = a.chains_npz or on_device
    if not have_libs and not (own_chains and a.no_plots and not point):
        sys.exit("run_BnpC.py: no vendored BnpC at %s (--bnpc_libs DIR): the reference's sampler, -e ML|MAP and the plots are the checkout's; only --chains_npz or "
                 "--sampler device / device-sm / device-errors, with --no_plots, run without one" % libs_dir)
    io = ut = None
    if have_libs:
        sys.path.insert(0, os.path.dirname(os.path.abspath(libs_dir)))
        import libs.dpmmIO as io
        import libs.utils as ut
    if io is not None:
        io.process_sim_folder(a, suffix="")
    data, names = bnpc.load_data(a.input, transpose=a.transpose)
    assert data.size > 0, f"Could not read data from file: {a.input}"
    a.time = [datetime.now()]
    if a.chains_npz:
        results = bnpc.load_chains(a.chains_npz)
    elif on_device:
        if a.debug:
            a.chains = 1
        results = _device_chains(a, data)
    else:
        from libs.MCMC import MCMC
        if a.falsePositive > 0 and a.falseNegative > 0:                      # run_BnpC.py:261-296
            a.error_update_prob = 0
            import libs.CRP as CRP
            model = CRP.CRP(data, DP_alpha=a.DPa_prior, param_beta=a.param_prior, FN_error=a.falseNegative, FP_error=a.falsePositive)
        else:
            import libs.CRP_learning_errors as CRP
            model = CRP.CRP_errors_learning(data, DP_alpha=a.DPa_prior, param_beta=a.param_prior, FP_mean=a.falsePositive_mean, FP_sd=a.falsePositive_std,
                                            FN_mean=a.falseNegative_mean, FN_sd=a.falseNegative_std)
        run_var, run_str = io._get_mcmc_termination(a)
        mcmc = MCMC(model, sm_prob=a.split_merge_prob, dpa_prob=a.conc_update_prob, error_prob=a.error_update_prob, sm_ratios=a.split_merge_ratios, sm_steps=a.split_merge_steps)
        if a.verbosity > 0:
            print(model); print(mcmc); print(f"Run MCMC with ({a.chains} chains {run_str}):")
        if a.debug:
            a.chains = 1
        mcmc.run(run_var, a.seed, a.chains, a.verbosity, a.fixed_assignment, a.debug)
        a.chain_seeds = mcmc.get_seeds()
        results = mcmc.get_results()
    a.time.append(datetime.now())
    if a.save_chains:
        bnpc.save_chains(a.save_chains, results)

    # dpmmIO._infer_results (:199-225) with the posterior estimate taken from the device
    if ut is not None:
        a.PSRF = ut.get_lugsail_batch_means_est([(r["ML"], r["burn_in"]) for r in results])
    else:
        from . import bnpc_sampler
        a.PSRF = bnpc_sampler.lugsail_psrf([(r["ML"], r["burn_in"]) for r in results])
    a.steps = [r["ML"].size for r in results]
    cat = bnpc.concat_chains(results)
    inferred = {"mean": {}}
    for est in a.estimator:
        if est != "posterior":
            inferred["mean"][est] = ut.get_latents_point(results, est, data, False)[0]
        elif a.host_estimate:
            inferred["mean"][est] = bnpc.posterior_estimate_host(cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"])
        else:
            with Engine(a.device) as eng:
                inferred["mean"][est] = bnpc.posterior_estimate(eng, cat["assignments"], cat["params"], data, cat["DP_alpha"], cat["FN"], cat["FP"],
                                                                linkage="scipy" if a.scipy_linkage else "device")
    out_dir = bnpc.out_dir_of(a.output, a.input, f"{a.time[0]:%Y%m%d_%H:%M:%S}")
    if a.verbosity > 0 and io is not None and not a.chains_npz:
        io.show_MCMC_summary(a, results)
        io.show_assignments(inferred, names[0])
        io.show_latents(inferred)
    if a.verbosity > 0:
        print(f"\nWriting output to: {out_dir}\n")
    bnpc.save_errors(inferred, a.estimator, a.chains, out_dir)
    bnpc.save_assignments(inferred, a.estimator, a.chains, out_dir)
    bnpc.save_geno(inferred, out_dir, names[1])
    if io is not None:
        if a.true_clusters:
            true_assign = io.load_txt(a.true_clusters)
            io.save_v_measure(inferred, true_assign, out_dir)
            io.save_ARI(inferred, true_assign, out_dir)
        data_plot = data
        if a.true_data:
            data_plot = io.load_data(a.true_data, transpose=a.transpose)
            io.save_hamming_dist(inferred, data_plot, out_dir)
        if not a.no_plots:
            io.save_geno_plots(a, inferred, data_plot, out_dir, names)          # the rule's declared output: genoCluster_posterior_mean_raw.pdf
            if data.shape[0] < 300:
                io.save_similarity(a, inferred, results, out_dir)
        if not a.chains_npz:
            for k in ("bnpc_libs", "save_chains", "chains_npz", "host_estimate", "device", "sampler"):      # args.txt lists the reference's arguments
                vars(a).pop(k)
            io.save_config(a, out_dir)


def celltype_reannotation(argv=None):
    """CellTypeReannotation.py --SNVs --fusions --outfile --meta [--min_variants --min_frac]  (:67-77)."""
    from . import reanno
    ap = argparse.ArgumentParser(description="Cancer / non-cancer re-annotation of the cells from their HCCV genotypes")
    ap.add_argument("--SNVs", required=True); ap.add_argument("--fusions", required=True); ap.add_argument("--outfile", required=True)
    ap.add_argument("--meta", required=True); ap.add_argument("--min_variants", type=int, default=3); ap.add_argument("--min_frac", type=float, default=0.2)
    a = ap.parse_args(argv)
    print("Outfile: ", a.outfile, "\n")
    reanno.celltype_reannotation(a.SNVs, a.fusions, a.meta, a.outfile, a.min_variants, a.min_frac)


def _add_gnomad_flag(ap):
    ap.add_argument("--allow_missing_gnomad", action="store_true", help="run without the gnomAD filter when the named source cannot be read (default: stop, as the reference does)")


def _apply_gnomad_flag(a):
    if getattr(a, "allow_missing_gnomad", False):
        os.environ["LONGSOM_ALLOW_MISSING_GNOMAD"] = "1"


def _gnomad_source(a):
    """the gnomAD source of a fused run: a prepared set (--gnomAD_set, `gnomad_set` below: no database is opened) before --gnomAD_json before
    --gnomAD_db"""
    return a.gnomAD_set or a.gnomAD_json or a.gnomAD_db or None


def gnomad_set(argv=None):
    """--gnomAD_db SRC --out FILE.npz --af_floor F: scans a gnomAD source (a gnomad_db directory / sqlite file or a JSON table) once and
    writes its one-base alleles with AF >= F as a prepared set (calling.GnomadSet) for --gnomAD_set; a run may then ask for any
    --max_gnomad_vaf >= F."""
    ap = argparse.ArgumentParser(description="Prepare the allele set of step 2's gnomAD filter from a gnomAD source")
    ap.add_argument("--gnomAD_db", required=True); ap.add_argument("--out", required=True); ap.add_argument("--af_floor", type=float, default=0.01)
    a = ap.parse_args(argv)
    if not a.out.endswith(".npz"):
        ap.error("--out must end in .npz (what --gnomAD_set recognises a prepared set by)")
    t0 = time.time()
    n = calling.write_gnomad_set(calling.open_gnomad(a.gnomAD_db, False), a.out, a.af_floor)
    print(json.dumps({"out": a.out, "alleles": n, "af_floor": a.af_floor, "seconds": time.time() - t0}))


def _add_htslib_flag(ap):
    ap.add_argument("--htslib_legacy_del_merge", action="store_true",
                    help="count the first column of a deletion that is followed by another deletion (CIGAR 1D2D) as 'D', as pysam over htslib <= 1.10 "
                         "does; default: htslib >= 1.11 ('O').  The reference's conda environment pins neither (workflow/envs/SComatic.yaml:9,23)")


def _apply_htslib_flag(a):
    if getattr(a, "htslib_legacy_del_merge", False):
        hostio.set_legacy_del_merge(True)


def _optional_paths(ap, *flags):
    """File options a rule may render with an EMPTY value (`--pon_LR {input.pon_LR}` when Run.PoN is False, the reference's
    default config): like the reference's own `--pon_LR` (step2.py:245, nargs='?'), a bare flag means "no file"."""
    for f in flags:
        ap.add_argument(f, nargs="?", const="", default="")


def _add_dataclass_flags(ap, obj, prefix=""):
    for k, v in vars(obj).items():
        if isinstance(v, bool):
            ap.add_argument("--" + prefix + k, action="store_true")
        elif isinstance(v, (int, float, str)):
            ap.add_argument("--" + prefix + k, type=type(v), default=v)


def snv(argv=None):
    """Fused chain: one process from BAM to calling.step3.tsv (workflow/rules/SNVCalling.gpu.smk)."""
    ap = argparse.ArgumentParser(description="SplitBam -> BaseCellCounter -> MergeCounts -> BaseCellCalling step1-3 on one GPU")
    ap.add_argument("--bam", required=True); ap.add_argument("--meta", required=True); ap.add_argument("--ref", required=True)
    ap.add_argument("--id", required=True); ap.add_argument("--outdir", required=True)
    _optional_paths(ap, "--editing", "--pon_SR", "--pon_LR", "--gnomAD_json", "--gnomAD_db", "--gnomAD_set")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--window_gb", type=float, default=0.0, help="stream the BAM in batches of about this many GiB of uncompressed BAM and count "
                    "window by window (for a BAM whose reads do not fit in HBM); 0 = the whole BAM at once")
    # SplitBamCellTypes' read filters, with its names and defaults (SplitBamCellTypes.py:199-202); not SnvParams fields, so that the flag
    # surfaces of `reannotation` and `pon` stay as they are
    ap.add_argument("--max_nM", type=_limit, default=None); ap.add_argument("--max_NH", type=_limit, default=None); ap.add_argument("--n_trim", type=int, default=0)
    # the CNA branch's cell-by-gene read counts from the same load (cli.gene_counts has the flags' meaning); off without --gene_counts_gtf
    ap.add_argument("--gene_counts_gtf", default="", help="also write {gene_counts_out}/{id}.counts.formated.txt from the load this chain holds")
    ap.add_argument("--gene_counts_out", default="", help="its directory (default: {outdir}/InferCNV/featurecount/output)")
    ap.add_argument("--gene_counts_names", default="third"); ap.add_argument("--gene_counts_tsv", action="store_true")
    d = pipeline.SnvParams()
    _add_dataclass_flags(ap, d)
    _add_htslib_flag(ap); _add_gnomad_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a); _apply_gnomad_flag(a)
    params = pipeline.SnvParams(**{k: getattr(a, k) for k in vars(d)})
    gene_counts = None
    if a.gene_counts_gtf:
        from . import genecounts
        if a.gene_counts_names not in genecounts.NAME_RULES:
            ap.error("--gene_counts_names %s: one of %s" % (a.gene_counts_names, ", ".join(genecounts.NAME_RULES)))
        gene_counts = genecounts.Request(a.gene_counts_gtf, a.gene_counts_out or os.path.join(a.outdir, "InferCNV", "featurecount", "output"),
                                         gene_names=a.gene_counts_names, tsv=a.gene_counts_tsv)
    # under torch.distributed.run (WORLD_SIZE > 1): one rank per GPU, regions sharded over the ranks; the process group comes up
    # before anything touches the GPU
    from . import regions
    comm = regions.Comm.from_env()
    try:
        out = pipeline.run_snv(a.bam, a.meta, a.ref, a.outdir, a.id, params, a.editing or None, a.pon_SR or None, a.pon_LR or None,
                               _gnomad_source(a), a.device, comm=comm, window_bytes=int(a.window_gb * (1 << 30)) or None,
                               filters=pipeline.SplitFilters(a.max_nM, a.max_NH, a.n_trim), gene_counts=gene_counts)
        if comm.rank == 0:
            print(json.dumps({"outputs": {k: v for k, v in vars(out).items() if k not in ("timings", "resident", "_pending")}, "seconds": out.timings, "ranks": comm.world}))
    finally:
        comm.close()


def reannotation(argv=None):
    """Fused two-pass loop: pass-1 calling, HCCV, per-cell genotyping, re-annotation, pass-2 calling; the BAM is decoded and loaded
    once (workflow/rules/CellTypeReannotation.gpu.smk)."""
    ap = argparse.ArgumentParser(description="CellTypeReannotation + SNVCalling of LongSom on one GPU, reads resident across both passes")
    ap.add_argument("--bam", required=True); ap.add_argument("--meta", required=True); ap.add_argument("--ref", required=True)
    ap.add_argument("--id", required=True); ap.add_argument("--outdir", required=True)
    _optional_paths(ap, "--fusions", "--editing", "--pon_SR", "--pon_LR", "--gnomAD_json", "--gnomAD_db", "--gnomAD_set")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--pass1_step3", action="store_true", help="also write pass 1's calling.step3.tsv (the reference's pass 1 stops at step 2)")
    # config['Reanno'] (pass 1: --reanno_* for the HCCV / re-annotation block, --p1_* for its BaseCellCounter / BaseCellCalling
    # block) and config['SNVCalling'] (pass 2: --p2_*); defaults = config/config.yaml
    rp0, sp0 = pipeline.ReannoParams(), pipeline.SnvParams()
    _add_dataclass_flags(ap, rp0, "reanno_"); _add_dataclass_flags(ap, rp0.chain, "p1_"); _add_dataclass_flags(ap, sp0, "p2_")
    _add_htslib_flag(ap); _add_gnomad_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a); _apply_gnomad_flag(a)
    chain = pipeline.SnvParams(**{k: getattr(a, "p1_" + k) for k in vars(rp0.chain)})
    rp = pipeline.ReannoParams(chain=chain, **{k: getattr(a, "reanno_" + k) for k, v in vars(rp0).items() if k != "chain"})
    sp = pipeline.SnvParams(**{k: getattr(a, "p2_" + k) for k in vars(sp0)})
    # under torch.distributed.run (WORLD_SIZE > 1): one rank per GPU, every rank keeps its region's reads resident across both passes
    from . import regions
    comm = regions.Comm.from_env()
    try:
        out = pipeline.run_reannotation(a.bam, a.meta, a.ref, a.outdir, a.id, rp, sp, fusions_tsv=a.fusions or None, editing=a.editing or None,
                                        pon_sr=a.pon_SR or None, pon_lr=a.pon_LR or None, gnomad_af_json=_gnomad_source(a), device=a.device,
                                        pass1_step3=a.pass1_step3, comm=comm)
        if comm.rank == 0:
            print(json.dumps({"hccv": out.hccv, "genotype": out.genotype, "barcodes": out.barcodes, "cells_kept": out.n_cells_kept, "cancer_cells": out.n_cancer,
                              "pass2_step3": out.pass2.step3 if out.pass2 else None, "seconds": out.timings, "ranks": comm.world}))
    finally:
        comm.close()


def pon(argv=None):
    """PoN.py --in_tsv LIST --out_file OUT [--min_samples 2] [--rm_prefix Yes|No]  (scripts/PoN/PoN.py:10-16)."""
    from . import pon as _pon
    ap = argparse.ArgumentParser(description="Script to build a SComatic Panel Of Normals (PoNs)")
    ap.add_argument("--in_tsv", required=True); ap.add_argument("--out_file", required=True)
    ap.add_argument("--min_samples", type=int, default=2); ap.add_argument("--rm_prefix", choices=["Yes", "No"], default="Yes")
    a = ap.parse_args(argv)
    print("-----------------------------------------------------------\n1. Building Panel Of Normals ...\n"
          "-----------------------------------------------------------\n")
    _pon.build_from_files(a.in_tsv, a.out_file, a.min_samples, a.rm_prefix)


def betabin_estimation(argv=None):
    """BetaBinEstimation.py --in_tsv LIST --outfile OUT [--n_sites 500000] [--seed 1992]  (scripts/PoN/BetaBinEstimation.py:154-160), fitted on
    the GPU from the listed BaseCellCounter tables (longsom_amd.bbfit).  --n_sites 0: every eligible site."""
    from . import bbfit
    ap = argparse.ArgumentParser(description="Script to estimate the Beta-binomial distribution parameters (alpha and beta) to be used afterwards in the BaseCellCalling.step1.py")
    ap.add_argument("--in_tsv", required=True); ap.add_argument("--outfile", required=True)
    ap.add_argument("--n_sites", type=int, default=500000); ap.add_argument("--seed", type=int, default=1992)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    paths = [l.rstrip("\n") for l in open(a.in_tsv)]
    paths = [p for p in paths if os.path.isfile(p)]          # :183-187
    print("\n- Number of tsv files to be used:\n  > ", len(paths))
    with Engine(a.device) as eng:
        est, infos, seen, kept = bbfit.fit_tables(eng, paths, a.n_sites, a.seed)
    print("\n- Sites: %d read, %d kept by the filter" % (seen, kept))
    for f, name in enumerate(("cell counts", "base counts")):
        print("\n- Beta-binomial estimation finished for %s (%d iterations):\n  > Alpha %d: %r\n  > Beta %d: %r"
              % (name, infos[f]["iterations"], f + 1, est[2 * f], f + 1, est[2 * f + 1]))
    bbfit.write_estimates(a.outfile, est)
    print("\n- Beta-binomial estimation report saved in:\n  > ", a.outfile)


def pon_chain(argv=None):
    """rules/PoN.smk SplitBam_PoN .. PoN fused: --normals is a TSV of id, bam, barcodes.tsv (workflow/rules/PoN.gpu.smk)."""
    ap = argparse.ArgumentParser(description="Panel of normals of LongSom on one GPU: count + step-1 call of every normal, then the PoN table")
    ap.add_argument("--normals", required=True); ap.add_argument("--ref", required=True); ap.add_argument("--outdir", required=True)
    ap.add_argument("--alpha1", type=float); ap.add_argument("--beta1", type=float)
    ap.add_argument("--alpha2", type=float); ap.add_argument("--beta2", type=float)
    ap.add_argument("--fit", action="store_true", help="fit the four beta-binomial parameters from the normals' count rows (BetaBinEstimation.py without R) and write "
                    "<outdir>/PoN/PoN/BetaBinEstimates.txt; --alpha1 .. --beta2 are not read")
    ap.add_argument("--fit_n_sites", type=int, default=0, help="BetaBinEstimation.py's --n_sites; 0 (default): every eligible site")
    ap.add_argument("--fit_seed", type=int, default=1992)
    ap.add_argument("--min_ac_cells", type=int, default=1); ap.add_argument("--min_ac_reads", type=int, default=1)
    ap.add_argument("--min_cells", type=int, default=1); ap.add_argument("--min_cell_types", type=int, default=1)
    ap.add_argument("--min_mq", type=int, default=60); ap.add_argument("--min_samples", type=int, default=1)
    ap.add_argument("--rm_prefix", choices=["Yes", "No"], default="No"); ap.add_argument("--no_tables", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    _add_htslib_flag(ap)
    a = ap.parse_args(argv)
    _apply_htslib_flag(a)
    bb = {k: getattr(a, k) for k in ("alpha1", "beta1", "alpha2", "beta2")}
    if a.fit:
        bb = {}
    elif any(v is None for v in bb.values()):
        ap.error("the following arguments are required: --alpha1, --beta1, --alpha2, --beta2 (or --fit)")
    normals = [tuple(l.rstrip("\n").split("\t")[:3]) for l in open(a.normals) if l.strip() and not l.startswith("#")]
    p = pipeline.pon_params(**bb, min_ac_cells=a.min_ac_cells, min_ac_reads=a.min_ac_reads,
                            min_cells=a.min_cells, min_cell_types=a.min_cell_types, min_mapping_quality=a.min_mq)
    # under torch.distributed.run: the normals are spread over the ranks (one GPU each)
    from . import regions
    comm = regions.Comm.from_env()
    try:
        out = pipeline.run_pon(normals, a.ref, a.outdir, p, a.min_samples, a.rm_prefix, not a.no_tables, device=a.device, comm=comm,
                               fit=a.fit, fit_n_sites=a.fit_n_sites, fit_seed=a.fit_seed)
        if comm.rank == 0:
            fitted = {"estimates": out.estimates, "estimates_file": out.estimates_path} if a.fit else {}
            print(json.dumps({"pon": out.pon, "sites": out.n_sites, "seconds": out.timings, "ranks": comm.world, **fitted}))
    finally:
        comm.close()


def main(argv=None):
    """python -m longsom_amd.cli <entry point> [flags]: the entry points above by name"""
    argv = sys.argv[1:] if argv is None else list(argv)
    names = sorted(n for n, f in globals().items() if callable(f) and not n.startswith("_") and getattr(f, "__module__", None) == __name__ and n != "main")
    if not argv or argv[0] not in names:
        sys.exit("usage: python -m longsom_amd.cli {%s} [flags]" % ",".join(names))
    globals()[argv[0]](argv[1:])


if __name__ == "__main__":
    main()
