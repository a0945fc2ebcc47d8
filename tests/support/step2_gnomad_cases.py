"""Installed count rows for the gnomAD filter's edge tests (tests/test_step2_gnomad_gpu.py): a few dozen sites over three contigs whose
string order is not their index order, made so that step 1 leaves every kind of row the filter tells apart - a bare PASS with a
one-base ALT, one-base rows with other FILTERs, "A|C" rows (two alternatives in one cell type) and "A,A" rows (the same alternative in
both cell types) - among them a site at the last position of the last contig."""
import numpy as np

NAMES = ["chr2", "chr10", "chrM"]                  # table order: chr10, chr2, chrM
LENS = [96, 70, 64]
CT_NAMES = ["Cancer", "Non-Cancer"]
_CLS = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3}


def sequences():
    rng = np.random.default_rng(2024)
    return [rng.choice(np.frombuffer(b"ACGT", np.uint8), n) for n in LENS]


def _row(ref_cls: int, ref_reads: int, alts):
    """one count row: ref_reads reads of the reference base, alts = [(class offset 1..3 from the reference's, reads, cells)]"""
    bc = np.zeros(8, np.int64); cc = np.zeros(8, np.int64)
    bc[ref_cls] = ref_reads; cc[ref_cls] = min(ref_reads, 12)
    for step, reads, cells in alts:
        a = (ref_cls + step) % 4
        bc[a], cc[a] = reads, cells
    r = np.zeros(42, np.uint32)
    r[0] = bc.sum(); r[1] = max(14, int(cc.max()) + 2); r[2:10] = cc; r[10:18] = bc; r[18:26] = bc * 30; r[26:34] = bc // 2; r[34:42] = bc - bc // 2
    return r


# what a site carries per cell type: None = no row, else the alternatives of _row
_KINDS = [
    ([(1, 14, 7)], []),                            # one alternative in Cancer alone, Non-Cancer covered: a one-base ALT
    ([(2, 14, 7)], []),
    ([(1, 12, 6), (2, 11, 6)], []),                # two alternatives in Cancer: "A|C"
    ([(1, 14, 7)], [(1, 13, 7)]),                  # the same alternative in both cell types: "A,A"
    ([(3, 14, 7)], None),                          # Cancer alone has a row: Min_cell_types
    ([], []),                                      # no alternative at all
    ([(1, 3, 2)], []),                             # a weak alternative
    ([], [(2, 14, 7)]),                            # an alternative in Non-Cancer alone
]


def count_rows():
    """per cell type (keys, counts): every third position of every contig carries a site, the kinds above in turn; the last position of
    every contig carries a one-base site"""
    seqs = sequences()
    per_ct = [([], []), ([], [])]
    n = 0
    for t, L in enumerate(LENS):
        for pos in list(range(7, L - 8, 3)) + [L - 1]:
            kind = _KINDS[0] if pos == L - 1 else _KINDS[n % len(_KINDS)]
            n += 1
            for ct in range(2):
                if kind[ct] is None:
                    continue
                per_ct[ct][0].append((t << 32) | pos)
                per_ct[ct][1].append(_row(_CLS[int(seqs[t][pos])], 40, kind[ct]))
    return [(np.asarray(k, np.int64), np.stack(r)) for k, r in per_ct]
