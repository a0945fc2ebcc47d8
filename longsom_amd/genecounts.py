"""Cell-by-gene read counts: the expression matrix inferCNV reads.

Stands in for three rules of the reference's workflow/rules/CNACalling.smk:
  split_per_bc         :11-27   one BAM per barcode (split_by_bc.py) - not needed: a read's barcode is resident (read_cb)
  featureCount         :29-44   featureCounts -L -a <gtf> over those BAMs: exons by gene_id, unstranded, a read to the one gene its
                                blocks overlap (Assigned), to none (NoFeatures) or to several (Ambiguity)
  format_featureCount  :46-75   gene ids -> names, unnamed ids dropped, rows summed by name, to_csv
The reference's branch cannot run as it is written and featureCounts is not part of this project, so the contract is this module's own
statement (DESIGN.md §13 lists the divergences); `count` below - plain numpy - IS that statement, the device (csrc/genecounts.hip) is held
to it exactly.

The annotation is flattened on the host into sorted, disjoint ELEMENTARY intervals (key = tid << 32 | start0, len, label): between two
neighbouring exon boundaries the set of covering genes is constant, so the label is that one gene's index or AMBIG for two and more.  A
read's blocks are its segments (runs of reference positions cut at N); a block asks one binary search and a short walk.
"""
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

AMBIG = 0xFFFFFFFE                 # label of an elementary interval that exons of two or more genes cover
OUTCOMES = ("Assigned", "NoFeatures", "Ambiguity", "Filtered")      # the columns of the tallies
NAME_RULES = ("third", "gene_name", "none")
FLAG_EXCLUDE = 0x4                 # featureCounts without --primary: every mapped record counts, on its own
FLAG_PRIMARY_ONLY = 0x900          # --primary_only adds secondary and supplementary


def _gtf_lines(path: str):
    """(line number, the 9 fields) of every non-comment line of a GTF that has 9 tab-separated fields"""
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if line.startswith("#"):
                continue
            parts = line.rstrip("\r\n").split("\t")
            if len(parts) == 9:
                yield no, parts


_GENE_ID = re.compile(r'(?:^|;)\s*gene_id\s+"([^"]*)"')


@dataclass
class Exons:
    """the `exon` lines of a GTF (featureCounts -t exon -g gene_id -s 0): gene index in order of first appearance, contig name, [start0, end0)"""
    gene_ids: List[str]
    gene: np.ndarray               # int64 [n]
    contig: List[str]              # [n]
    start0: np.ndarray             # int64 [n]
    end0: np.ndarray               # int64 [n]


def read_exons(path: str) -> Exons:
    ids: Dict[str, int] = {}
    gene, contig, s0, e0 = [], [], [], []
    for no, p in _gtf_lines(path):
        if p[2] != "exon":
            continue
        m = _GENE_ID.search(p[8])
        if not m:
            raise ValueError("%s line %d: an exon without a gene_id attribute" % (path, no))
        start, end = int(p[3]), int(p[4])
        if start < 1 or end < start:
            raise ValueError("%s line %d: exon [%d, %d]" % (path, no, start, end))
        gene.append(ids.setdefault(m.group(1), len(ids))); contig.append(p[0]); s0.append(start - 1); e0.append(end)      # 1-based inclusive -> [start - 1, end)
    return Exons(list(ids), np.asarray(gene, np.int64), contig, np.asarray(s0, np.int64), np.asarray(e0, np.int64))


def read_name_map(path: str, rule: str = "third") -> Dict[str, str]:
    """gene_id -> name from the `gene` lines of a GTF, a later line winning.  third: the first quoted string of attribute field 0 -> that
    of field 2 (format_featureCount's gene_name_dico, CNACalling.smk:55-62: gene_type sits between them in GENCODE); gene_name: the
    attribute of that name."""
    if rule not in ("third", "gene_name"):
        raise ValueError("no name map for --gene_names %s" % rule)
    out: Dict[str, str] = {}
    for no, p in _gtf_lines(path):
        if p[2] != "gene":
            continue
        fields = p[8].split(";")
        try:
            gid = fields[0].split('"')[1]
            if rule == "third":
                name = fields[2].split('"')[1]
            else:
                m = re.search(r'(?:^|;)\s*gene_name\s+"([^"]*)"', p[8])
                if not m:
                    continue                                  # no such attribute: the id has no name
                name = m.group(1)
        except IndexError:
            raise ValueError("%s line %d: a gene line without a quoted %s attribute field" % (path, no, "third" if rule == "third" else "first")) from None
        out[gid] = name
    return out


@dataclass
class Annotation:
    """the flattened exons: what lsg_load_annotation takes"""
    gene_ids: List[str]
    keys: np.ndarray               # uint64 [n_iv]  tid << 32 | start0, ascending
    lens: np.ndarray               # uint32 [n_iv]
    labels: np.ndarray             # uint32 [n_iv]  gene index or AMBIG
    n_dropped_exons: int = 0       # exons on contigs the BAM does not have

    @property
    def n_genes(self): return len(self.gene_ids)
    @property
    def n_intervals(self): return len(self.keys)


def flatten(exons: Exons, contig_names: Sequence[str]) -> Annotation:
    """Sweep every contig's exon boundaries: a piece between two neighbouring boundaries that at least one exon covers is one elementary
    interval (pieces are not merged: a piece IS the unit the label is constant on).  Contig names match the BAM header's exactly."""
    tid_of = {n: i for i, n in enumerate(contig_names)}
    tid = np.asarray([tid_of.get(c, -1) for c in exons.contig], np.int64)
    have = tid >= 0
    keys, lens, labels = [], [], []
    for t in np.unique(tid[have]):
        sel = np.nonzero(tid == t)[0]
        ev = sorted([(int(exons.start0[i]), 1, int(exons.gene[i])) for i in sel] + [(int(exons.end0[i]), 0, int(exons.gene[i])) for i in sel])      # at one position ends come first
        active: Dict[int, int] = {}
        prev = 0
        for pos, opens, g in ev:
            if pos > prev and active:
                keys.append((int(t) << 32) | prev); lens.append(pos - prev)
                labels.append(next(iter(active)) if len(active) == 1 else AMBIG)
            prev = pos
            if opens:
                active[g] = active.get(g, 0) + 1
            elif active[g] == 1:
                del active[g]
            else:
                active[g] -= 1
    if any((k & 0xFFFFFFFF) + l > 1 << 32 for k, l in zip(keys, lens)):
        raise ValueError("an exon ends past position 2^32")
    return Annotation(exons.gene_ids, np.asarray(keys, np.uint64), np.asarray(lens, np.uint32), np.asarray(labels, np.uint32), int((~have).sum()))


def load_annotation(gtf: str, contig_names: Sequence[str]) -> Annotation:
    return flatten(read_exons(gtf), contig_names)


_BAD_NAME = re.compile('[,"\t\r\n]')


def rows_of(gene_ids: Sequence[str], names: Optional[Dict[str, str]]) -> Tuple[List[str], np.ndarray]:
    """(row names sorted by code point, row_of_gene int32 [n_genes], -1 = the id has no name and leaves the file): df['Geneid'].map(dico),
    notnull, groupby('Geneid') (CNACalling.smk:69-71).  names None: the ids are the rows (--gene_names none).  A name the file's plain
    separator-joined rows cannot hold is refused."""
    named = [g if names is None else names.get(g) for g in gene_ids]
    for n in named:
        if n is not None and _BAD_NAME.search(n):
            raise ValueError("gene name %r holds a comma, a quote, a tab or a line break: the matrix is written without CSV quoting" % n)
    rows = sorted(set(n for n in named if n is not None))
    at = {n: i for i, n in enumerate(rows)}
    return rows, np.asarray([-1 if n is None else at[n] for n in named], np.int32)


def column_order(barcodes: Sequence[str]) -> np.ndarray:
    """the columns: every barcode of the table in byte order of its string (the *.bam glob order of the reference's per-barcode files)"""
    return np.asarray(sorted(range(len(barcodes)), key=lambda i: barcodes[i].encode()), np.int32)


def read_states(rec, ann: Annotation, considered: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """per read (lo, hi) = (smallest gene index its blocks overlap, largest + 1), an ambiguous interval counting as genes 0 and 2^32 - 2:
    none (0xFFFFFFFF, 0), one gene hi == lo + 1, else ambiguous - the two words the segment kernel folds with atomicMin / atomicMax"""
    R = rec.n_reads
    lo = np.full(R, 0xFFFFFFFF, np.uint32); hi = np.zeros(R, np.uint32)
    if rec.n_segs == 0 or ann.n_intervals == 0:
        return lo, hi
    r = rec.seg_read.astype(np.int64)
    ok = considered[r] & (rec.seg_len > 0) & (rec.read_tid[r] >= 0)
    r = r[ok]
    ks = (rec.read_tid[r].astype(np.uint64) << np.uint64(32)) + rec.seg_start[ok].astype(np.uint64)
    ke = ks + rec.seg_len[ok].astype(np.uint64)
    ends = ann.keys + ann.lens.astype(np.uint64)            # ascending as well: the intervals are disjoint
    i0 = np.searchsorted(ends, ks, side="right")            # the first interval that ends after the block's start
    i1 = np.searchsorted(ann.keys, ke, side="left")         # ... and the first that starts at or after its end
    n = np.maximum(i1 - i0, 0)
    hit_read = np.repeat(r, n)
    idx = np.repeat(i0 - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
    lab = ann.labels[idx]
    amb = lab == AMBIG
    np.minimum.at(lo, hit_read, np.where(amb, 0, lab).astype(np.uint32))
    np.maximum.at(hi, hit_read, np.where(amb, 0xFFFFFFFF, lab.astype(np.uint64) + 1).astype(np.uint32))
    return lo, hi


def count_genes(rec, ann: Annotation, n_cb: int, min_mapq: int = 0, flag_exclude: int = FLAG_EXCLUDE):
    """The contract.  Returns (per gene id: int64 [n_genes][n_cb] reads assigned, tallies int64 [n_cb][4] in OUTCOMES order)."""
    cb = rec.read_cb.astype(np.int64)
    listed = (cb >= 0) & (cb < n_cb)
    considered = listed & ((rec.read_flag.astype(np.int64) & int(flag_exclude)) == 0) & (rec.read_mapq.astype(np.int64) >= int(min_mapq))
    lo, hi = read_states(rec, ann, considered)
    none = considered & (hi == 0)
    one = considered & (hi == lo.astype(np.uint64) + 1) & ~none
    tallies = np.zeros((n_cb, 4), np.int64)
    for col, mask in enumerate((one, none, considered & ~one & ~none, listed & ~considered)):
        tallies[:, col] = np.bincount(cb[mask], minlength=n_cb)
    per_gene = np.zeros((ann.n_genes, n_cb), np.int64)
    np.add.at(per_gene, (lo[one].astype(np.int64), cb[one]), 1)
    return per_gene, tallies


def count(rec, ann: Annotation, row_of_gene: np.ndarray, n_rows: int, n_cb: int, min_mapq: int = 0, flag_exclude: int = FLAG_EXCLUDE):
    """(matrix int64 [n_rows][n_cb] in barcode-id order, tallies [n_cb][4]): count_genes with the ids' rows summed by name"""
    per_gene, tallies = count_genes(rec, ann, n_cb, min_mapq, flag_exclude)
    matrix = np.zeros((n_rows, n_cb), np.int64)
    keep = row_of_gene >= 0
    np.add.at(matrix, row_of_gene[keep], per_gene[keep])
    return matrix, tallies


def matrix_text(matrix: np.ndarray, row_names: Sequence[str], barcodes: Sequence[str], order: np.ndarray, sep: str = ",") -> bytes:
    """DataFrame.to_csv of the formatted table: `Geneid,<bc>,...` then `<name>,<int>,...`, the columns in `order`"""
    m = np.asarray(matrix)[:, order] if len(row_names) else np.zeros((0, len(order)), np.int64)
    lines = [sep.join(["Geneid"] + [barcodes[i] for i in order])]
    lines += [sep.join([name] + [str(int(v)) for v in row]) for name, row in zip(row_names, m)]
    return ("\n".join(lines) + "\n").encode()


def summary_text(tallies: np.ndarray, barcodes: Sequence[str], order: np.ndarray) -> bytes:
    """{id}.counts.summary.tsv: one row per outcome, a column per barcode (the shape of featureCounts' .summary)"""
    lines = ["\t".join(["Status"] + [barcodes[i] for i in order])]
    lines += ["\t".join([name] + [str(int(tallies[i, k])) for i in order]) for k, name in enumerate(OUTCOMES)]
    return ("\n".join(lines) + "\n").encode()


def name_rows(ann: Annotation, gtf: str, names_gtf: Optional[str], rule: str):
    if rule not in NAME_RULES:
        raise ValueError("--gene_names %s: one of %s" % (rule, ", ".join(NAME_RULES)))
    return rows_of(ann.gene_ids, None if rule == "none" else read_name_map(names_gtf or gtf, rule))


def device_matrix(eng, ann: Annotation, row_names, row_of_gene, barcodes, order, sep: str, min_mapq: int, flag_exclude: int, out_path: Optional[str] = None):
    """The resident load counted on the device and the matrix printed there: lsg_load_annotation, lsg_gene_counts, lsg_gene_counts_set_text,
    LSG_TABLE_GENE_COUNTS.  out_path: the text is streamed into that file (lsg_append_table) and not returned.  Returns (info, tallies
    [n_cb][4], text or None); the annotation and the matrix are freed again."""
    eng.gene_counts_reset()
    try:
        eng.load_annotation(ann, row_of_gene, len(row_names))
        info = eng.gene_counts(min_mapq, flag_exclude)
        eng.gene_counts_set_text(row_names, order, barcodes, sep)
        n = eng.format_table(eng.TABLE_GENE_COUNTS)
        text = None
        if out_path is None:
            text = eng.table_bytes(eng.TABLE_GENE_COUNTS, n)
        else:
            open(out_path, "wb").close()
            eng.append_table(eng.TABLE_GENE_COUNTS, out_path)
        _, tallies = eng.gene_counts_fetch(matrix=False)
        return info, tallies, text
    finally:
        eng.gene_counts_reset()


@dataclass
class Request:
    """what pipeline.run_snv(gene_counts=...) makes from the load it holds: cli.gene_counts' flags"""
    gtf: str
    out_dir: str
    names_gtf: Optional[str] = None
    gene_names: str = "third"
    tsv: bool = False
    min_mapq: int = 0
    primary_only: bool = False


def run_resident(eng, contig_names: Sequence[str], barcodes: Sequence[str], req: Request, sample_id: str) -> Tuple[str, str]:
    """{out_dir}/{id}.counts.formated.txt and .counts.summary.tsv from the reads resident in `eng` (loaded against `barcodes`, under no
    load filter stricter than the request's); reads and changes nothing of the store, the count rows or the calls"""
    ann = load_annotation(req.gtf, contig_names)
    rows, row_of_gene = name_rows(ann, req.gtf, req.names_gtf, req.gene_names)
    order = column_order(barcodes)
    os.makedirs(req.out_dir, exist_ok=True)
    out = os.path.join(req.out_dir, sample_id + ".counts.formated.txt")
    _, tallies, _ = device_matrix(eng, ann, rows, row_of_gene, barcodes, order, "\t" if req.tsv else ",", req.min_mapq,
                                  FLAG_EXCLUDE | (FLAG_PRIMARY_ONLY if req.primary_only else 0), out_path=out)
    return write_outputs(req.out_dir, sample_id, None, tallies, barcodes, order)


def write_outputs(out_dir: str, sample_id: str, text: Optional[bytes], tallies, barcodes, order) -> Tuple[str, str]:
    os.makedirs(out_dir, exist_ok=True)
    counts = os.path.join(out_dir, sample_id + ".counts.formated.txt")
    summary = os.path.join(out_dir, sample_id + ".counts.summary.tsv")
    if text is not None:
        with open(counts, "wb") as f:
            f.write(text)
    with open(summary, "wb") as f:
        f.write(summary_text(tallies, barcodes, order))
    return counts, summary
