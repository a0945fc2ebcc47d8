/*
 * longsom_hip.h — C-ABI of liblongsom_hip.so, the MI355X (gfx950) implementation of
 * LongSom's SComatic-derived SNV hot path:
 *
 *   SplitBamCellTypes -> BaseCellCounter -> MergeBaseCellCounts -> BaseCellCalling.step1
 *
 * The reference has no FFI for this path (it is pure Python): the operator
 * boundary is the Snakemake rule contract (files in / files out).  This header is the boundary
 * a maintainer binds with ctypes from the rule scripts; each entry point
 * names the reference code it replaces (paths relative to /root/reference/workflow/scripts).
 *
 * Conventions
 *   - plain C, pointers + sizes only; no torch / C++ types.
 *   - every call returns 0 on success, <0 on error; lsg_last_error() gives the message
 *     (thread-local).  One handle per GPU; a handle is not thread-safe; handles are independent.
 *   - "on_device" != 0 means the array pointers are device pointers on the handle's GPU
 *     (e.g. torch tensors' data_ptr()); 0 means host memory; either way borrowed for the duration of the call
 *     (exception: lsg_load_reference adopts a device array).
 *   - positions are 0-based on the device; text writers add 1 (BaseCellCounter.py:288).
 *   - there is NO CPU fallback in this library: without a HIP device lsg_create() fails.
 */
#ifndef LONGSOM_HIP_H
#define LONGSOM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsg_ctx lsg_ctx;

/* Symbol classes of one pileup entry, in the allele order of the reference
 * (BaseCellCalling.step1.py:20  Alleles = ["A","C","T","G","I","D","N","O"]);
 * LSG_SYM_NA = the reference's 'NA' (intron '>' '<', IUPAC, '=': EasyReadPileup,
 * BaseCellCounter.py:152-180) and is never counted. */
enum { LSG_SYM_A = 0, LSG_SYM_C = 1, LSG_SYM_T = 2, LSG_SYM_G = 3, LSG_SYM_I = 4,
       LSG_SYM_D = 5, LSG_SYM_N = 6, LSG_SYM_O = 7, LSG_SYM_NA = 15 };

/* One count row = 42 uint32 per (site, cell type):
 *   [0] DP   [1] NC   [2..9] CC   [10..17] BC   [18..25] BQ   [26..33] BCf   [34..41] BCr
 * each vector indexed by the symbol class above (the TSV prints classes 0..5 only,
 * BaseCellCounter.py:300-306). */
#define LSG_EVENT_VALID 0x0800u
#define LSG_EVENT(sym, qual) ((uint16_t)((sym) < 8 ? (LSG_EVENT_VALID | ((sym) << 8) | ((qual) & 0xffu)) : 0u))
#define LSG_EVENT_SYM(ev) (((ev) & LSG_EVENT_VALID) ? (((ev) >> 8) & 7u) : (unsigned)LSG_SYM_NA)
#define LSG_EVENT_QUAL(ev) ((ev) & 0xffu)
#define LSG_ROW_WORDS 42
#define LSG_MAX_CELLTYPES 4

/* Pre-decoded read-record arrays ("SoA" form of a coordinate-sorted BAM).
 * A read is split into SEGMENTS = maximal runs of consecutive reference positions that carry a
 * pileup entry (M/=/X/D columns; N reference skips break segments).  One EVENT per covered
 * reference position: uint16 = LSG_EVENT(symbol_class, base_quality) = 0x0800 | class << 8 | quality for the
 * eight countable classes and 0 for LSG_SYM_NA (so that "no event" and "not countable" are both 0: the
 * kernels read lanes outside an entry's range as 0), where the symbol class and the
 * quality follow htslib bam_plp + pysam PileupColumn semantics as used by BaseCellCounter.py:191-216
 * (anchor base of an indel -> I / D, interior deletion column -> O with the quality of the next
 * query base). */
/* Where a segment's events lie in `events` is the producer's choice (seg_ev_off; n_events = the array's extent, gaps are never read).
 * Two layouts are made by this library's own producers (the device BAM decoder, the synthetic generators):
 *   LSG_LAYOUT_COMPACT  segment after segment, no gaps;
 *   LSG_LAYOUT_PHASED   "tile-phased": every read's region starts at a multiple of 128 events and every segment at an offset congruent
 *                       to its reference start modulo 128 (gaps hold 0), so that the events a read has inside one 128-position window of the
 *                       pileup (tiles 2 w and 2 w + 1) lie inside ONE aligned 256-byte block of the array, and those inside one 64-position
 *                       tile inside one aligned 128-byte line: the count fetches every block once, with one load instruction.
 * lsg_load_reads recognises a phased array by looking (every admitted segment's (seg_ev_off - seg_start) is a multiple of 64 / 128, `events`
 * is 128 / 256-byte aligned).  Whether it bins a load by windows or by tiles has to be decided before it has looked, though: a caller whose
 * arrays are phased modulo 128 says so with lsg_set_events_layout (this library's own producers do); a load that finds the claim wrong
 * starts again by tiles.  A caller's own arrays may use either layout, or anything else. */
enum { LSG_LAYOUT_COMPACT = 0, LSG_LAYOUT_PHASED = 1 };
typedef struct {
    int64_t n_reads;
    int64_t n_segs;
    int64_t n_events;
    /* per read */
    const int32_t*  read_tid;    /* contig index                                  */
    const int32_t*  read_pos;    /* 0-based leftmost position                     */
    const uint16_t* read_flag;   /* SAM flag                                      */
    const uint8_t*  read_mapq;   /* MAPQ                                          */
    const int32_t*  read_cb;     /* dense barcode id, -1 = no CB tag / not in barcodes.tsv */
    /* per segment */
    const uint32_t* seg_read;    /* owning read index                             */
    const int32_t*  seg_start;   /* 0-based reference start                       */
    const int32_t*  seg_len;     /* number of reference positions (= events)      */
    const int64_t*  seg_ev_off;  /* index of the segment's first event            */
    /* per event */
    const uint16_t* events;
    int32_t on_device;
} lsg_reads;

/* Parameters of the count stage; defaults = the flags LongSom's rules pass
 * (R:SNVCalling.smk:52-59 + script defaults BaseCellCounter.py:331-339). */
typedef struct {
    int32_t min_bq;        /* --min_bq  20 */
    int32_t min_mq;        /* --min_mq  60 (config.yaml:74) */
    int32_t min_dp;        /* --min_dp  5  */
    int32_t min_cc;        /* --min_cc  5  */
    uint32_t flag_exclude; /* reads with any of these SAM flag bits are dropped:
                              0x4|0x100|0x200|0x400 (pysam pileup flag_filter) | 0x800
                              (BaseCellCounter.py:249) = 0xF04 */
    int32_t ignore_orphans;/* 1: drop paired reads that are not proper pairs (pysam default) */
    int32_t max_depth;     /* bam.pileup(..., max_depth = 200000), BaseCellCounter.py:191 — htslib's bam_plp_push rule, applied to
                              every cell type's read stream (= its SplitBam output): a read that is not the first of its start
                              position is dropped while the reads still buffered (end >= that position, counting secondary-free,
                              MAPQ- and orphan-filtered reads INCLUDING supplementary ones) + 1 exceed max_depth.  0 = no cap.
                              Costs nothing while lsg_max_live_reads() <= max_depth (no read can be dropped then). */
} lsg_count_params;

/* Parameters of the step-1 call (BaseCellCalling.step1.py:585-604). */
typedef struct {
    double alpha1, beta1, alpha2, beta2;
    int32_t min_cov;        /* --min_cov 5        */
    int32_t min_cells;      /* --min_cells 5      */
    int32_t min_ac_cells;   /* --min_ac_cells 2   */
    int32_t min_ac_reads;   /* --min_ac_reads 3   */
    int32_t max_cell_types; /* --max_cell_types 1 */
    int32_t min_cell_types; /* --min_cell_types 2 */
} lsg_call_params;

/* One step-1 call record per merged site (fixed size; the host formats the TSV line).
 * p-values are stored as the integer k with p = k / 10000 after Python round(x, 4)
 * (round-half-even on the exact binary value). */
#define LSG_CALL_MAX_ALT 4   /* 4 when REF is not one of A,C,G,T (IUPAC reference base) */
typedef struct {
    int64_t  key;                       /* (tid << 32) | pos0                                   */
    uint8_t  ref;                       /* reference base (ASCII, upper)                        */
    uint8_t  present;                   /* bit c: cell type c has a count row at this site      */
    uint8_t  considered;                /* bit c: cell type c passed min_cov / min_cells         */
    uint8_t  has_cand;                  /* bit c: cell type c has >=1 alt candidate             */
    uint8_t  n_alt[LSG_MAX_CELLTYPES];  /* candidates per cell type                             */
    uint8_t  alt[LSG_MAX_CELLTYPES][LSG_CALL_MAX_ALT];    /* symbol class, sorted as 'A'<'C'<'G'<'T' */
    uint8_t  ct_filter[LSG_MAX_CELLTYPES];                /* enum lsg_ct_filter                  */
    uint32_t alt_bc[LSG_MAX_CELLTYPES][LSG_CALL_MAX_ALT];
    uint32_t alt_cc[LSG_MAX_CELLTYPES][LSG_CALL_MAX_ALT];
    int32_t  p_bc[LSG_MAX_CELLTYPES][LSG_CALL_MAX_ALT];   /* round(sf,4) * 1e4                   */
    int32_t  p_cc[LSG_MAX_CELLTYPES][LSG_CALL_MAX_ALT];
    uint32_t site_filter;               /* bit set, enum lsg_site_filter                        */
    int32_t  cell_types_min;            /* Cell_types_min_BC == Cell_types_min_CC               */
    int32_t  sum_alts_bc, sum_dp, sum_alts_cc, sum_nc;    /* Rest_BC / Rest_CC; sum_nc can be negative (step1.py:256) */
    int32_t  noise_p_bc, noise_p_cc;    /* round(1-cdf,4)*1e4; -1 when Sum_alts_bc == 0 (prints "1"); -2 = nan (negative n) */
    uint8_t  up_ctx[5], down_ctx[5];    /* ASCII; up_ctx[0]==0 => "." (POS < 6)                 */
    uint8_t  pad[2];
} lsg_call;

enum lsg_ct_filter { LSG_CF_NONE = 0, LSG_CF_NONSIG, LSG_CF_LOWSIG, LSG_CF_MULTI, LSG_CF_LOW_CELLS,
                     LSG_CF_LOW_READS, LSG_CF_PASS };
enum lsg_site_filter { LSG_SF_MULTIPLE_CELL_TYPES = 1, LSG_SF_MULTI_ALLELIC = 2, LSG_SF_MIN_CELL_TYPES = 4,
                       LSG_SF_CELL_TYPE_NOISE = 8, LSG_SF_NOISY_SITE = 16, LSG_SF_LC_UP = 32,
                       LSG_SF_LC_DOWN = 64, LSG_SF_CANDIDATE = 1u << 31 };

/* ---- lifetime -------------------------------------------------------------------------------*/
int         lsg_create(int device_id, lsg_ctx** out);
void        lsg_destroy(lsg_ctx* ctx);
const char* lsg_last_error(void);
const char* lsg_version(void);
/* Launch everything on this hipStream_t (pass torch.cuda.current_stream().cuda_stream);
 * NULL = the handle's own stream. */
int         lsg_set_stream(lsg_ctx* ctx, void* hip_stream);
int         lsg_synchronize(lsg_ctx* ctx);

/* ---- inputs ---------------------------------------------------------------------------------*/
/* Contig table = pysam.FastaFile.references / get_reference_length (BaseCellCounter.py:84-86). */
int lsg_set_contigs(lsg_ctx* ctx, int32_t n_contigs, const int64_t* lengths);
/* Upper-cased reference bases of one contig (inFasta.fetch(...).upper(), BaseCellCounter.py:202-203;
 * BaseCellCalling.step1.py:98-99). */
int lsg_load_reference(lsg_ctx* ctx, int32_t tid, const uint8_t* bases, int64_t len, int32_t on_device);
/* celltype_of[cb] in [0, n_celltypes) or 255 = barcode not used.  Replaces meta_to_dict + the
 * per-read routing of SplitBamCellTypes.py:16-36,83-90,173: a re-annotation pass only swaps this
 * table, the reads stay resident. */
int lsg_set_barcodes(lsg_ctx* ctx, const uint8_t* celltype_of, int32_t n_cb, int32_t n_celltypes);
/* Loads the read-record arrays: replaces reading the per-cell-type BAMs in run_interval (BaseCellCounter.py:190-191) AND the
 * pileup engine's transposition of reads into columns (bam.pileup -> htslib bam_plp, :191-198), done here once per load on the device.
 * The call builds the TILE STORE, the library's only resident form of the events: every (segment x 64-position tile) overlap of a
 * read that carries a barcode is one entry, the entries of a tile adjacent and sorted by barcode, eight entries to a 1 KB block held
 * transposed ([position][entry]); beside every entry its barcode, strand, SAM flag, MAPQ and owning read, so that every later
 * lsg_pileup_count (any parameters, any barcode table, any region) and lsg_genotype_cells run from the store alone.  Needs the
 * contigs (lsg_set_contigs).  The caller's arrays — host (on_device = 0) or device (1) — are free again when the call returns: the
 * per-read and per-segment arrays are copied, the events are read once.  Whatever offsets seg_ev_off holds is fine (segments may even
 * share events); a segment whose event range lies outside [0, n_events) or whose read index lies outside the reads is an error, and a
 * refused load leaves no reads behind.  Segments that do not lie inside their contig are never counted. */
int lsg_load_reads(lsg_ctx* ctx, const lsg_reads* reads);
/* Load filter: reads with MAPQ < min_mq, any SAM flag bit of flag_exclude, or (ignore_orphans) paired without proper pair are not
 * stored by the NEXT lsg_load_reads calls — what SplitBamCellTypes.py:110-113 does to the BAM before BaseCellCounter sees it
 * (LongSom passes the same min_MQ to both, R:SNVCalling.smk:22-27,52-59).  Default: none (0, 0, 0), every read with a barcode is
 * stored and any count parameters can be resolved later; with a filter the store is smaller by the dropped reads' share and a count or
 * genotyping pass whose own filters would admit a dropped read is refused.  The per-read arrays (depth cap, statistics) keep every read. */
int lsg_set_load_filter(lsg_ctx* ctx, int32_t min_mq, uint32_t flag_exclude, int32_t ignore_orphans);
/* What the caller knows about where the events of the NEXT lsg_load_reads calls lie: LSG_LAYOUT_PHASED = phased modulo 128 (lsg_reads above),
 * LSG_LAYOUT_COMPACT (default) = no promise.  A promise lets a load that keeps no store (lsg_set_store_policy) bin its entries by
 * 128-position windows; it is checked, and a load that finds it broken falls back by itself.  No reference counterpart. */
int lsg_set_events_layout(lsg_ctx* ctx, int32_t layout);
/* Device-side ingest of a whole BAM: the file's bytes in (host memory), the tile store out — BGZF inflate, record
 * chain, CB lookup, SplitBam's counters and the CIGAR walk all run on the GPU (csrc/ingest.hip), then lsg_load_reads on the device
 * arrays.  Replaces pysam.AlignmentFile + infile.fetch() + read.opt("CB") + the MAPQ counters of split_bam
 * (SplitBamCellTypes.py:51-124) and the record decode behind bam.pileup (BaseCellCounter.py:190-191).  Needs the contigs = the BAM
 * header's reference table (the caller parses the header: hostio.bam_header) and first_record_offset = the header's length in the
 * uncompressed stream.  barcodes: n_barcodes cleaned strings joined by '\n', ids[i] = dense id of barcode i (NULL: i); duplicated
 * strings: the last wins.  cb_pass / cb_low (may be NULL): per dense id, matched reads with MAPQ >= / < min_mapq (what the report of a
 * re-annotated table needs).  legacy_del_merge: htslib <= 1.10's 1D2D rule.  Returns -4 when the file's records
 * straddle its BGZF blocks so badly that the record chain did not settle (not written by htslib): decode such a file on the host. */
typedef struct {
    int64_t total_reads, pass_reads, cb_not_found, cb_not_matched, mapq_filtered;      /* {id}.report.txt, SplitBamCellTypes.py:181-187 */
    int64_t n_records, n_blocks, n_ubytes;
    float   ms_h2d, ms_inflate, ms_chain, ms_decode, ms_store, ms_total;               /* HIP-event / wall times of the phases */
    int32_t chain_rounds, pad_;
    int64_t last_key;           /* (tid << 32 | pos) of the last complete record, 2^63 - 1 for one without a reference, -1: no record */
} lsg_bam_info;
int lsg_load_bam(lsg_ctx* ctx, const uint8_t* file_bytes, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                 const int32_t* ids, int32_t min_mapq, int32_t legacy_del_merge, lsg_bam_info* info, int64_t* cb_pass, int64_t* cb_low, int64_t n_tally);
/* The same for a SLICE of a coordinate-sorted BAM — whole BGZF blocks cut out of the file, starting with a block in which a record starts
 * at first_record_offset (what the .bai's linear index gives: virtual offset = block start << 16 | offset in the block): what one rank of
 * a sharded run ingests, as the reference's workers fetch their window through the index (BaseCellCounter.py:190-191; the .bai is a
 * rule input, rules/SNVCalling.smk:6-7).  A record cut by the end of the slice is skipped.  SplitBam's counters and the per-barcode
 * tallies take only the records whose (tid << 32 | pos) lies in [count_lo_key, count_hi_key): neighbouring slices overlap (a rank
 * also needs the reads that reach into its region), the sum over the ranks counts every record once.  info->last_key tells the caller
 * whether the slice reached the first read starting at or after its region's end (every read before it in the file starts earlier:
 * nothing that overlaps the region is missing); if not it asks again with a longer slice (longsom_amd/regions.py). */
int lsg_load_bam_range(lsg_ctx* ctx, const uint8_t* slice_bytes, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                       const int32_t* ids, int32_t min_mapq, int32_t legacy_del_merge, int64_t count_lo_key, int64_t count_hi_key, lsg_bam_info* info,
                       int64_t* cb_pass, int64_t* cb_low, int64_t n_tally);
/* keep != 0: the next loads also keep a copy of the compact events (and seg_ev_off) beside the store, which is what
 * lsg_copy_reads_to_host returns (tests, sampling for a CPU baseline).  Default 0: the store is the only copy (2 B per event saved). */
int lsg_set_keep_reads(lsg_ctx* ctx, int32_t keep);
/* Gives back everything a load and its counts hold on the device (reads, the tile store, the build's cached temporaries, count rows,
 * call records): the handle is as after lsg_set_barcodes, ready for the next lsg_load_reads / lsg_load_bam.  What a worker process of the
 * reference does by ending (BaseCellCounter.py:392-402 starts a pool per BAM); here a long-lived handle moves from one sample to the next,
 * and a sample of C4's size (155 GB resident) needs the room of the one before it. */
int lsg_unload_reads(lsg_ctx* ctx);
/* The reference counts through bam.pileup(..., max_depth = 200000) (BaseCellCounter.py:191,
 * HCCVSingleCellGenotype.py:122): htslib stops admitting reads at a position while more than max_depth are
 * live in its buffer.  lsg_pileup_count models that cap exactly (lsg_count_params.max_depth); this call evaluates
 * the upper bound it uses to skip the work: the live reads of every cell-type BAM under the current barcode table
 * (reads of one cell type whose span touches a 64-position tile, maximum over tiles and cell types; before
 * lsg_set_barcodes: all reads with a barcode).  While the bound stays <= max_depth the cap cannot fire.
 * lsg_genotype_cells_grouped models it for the genotyping pileup of the unsplit BAM (HCCVSingleCellGenotype.py:122) with the all-reads
 * bound (lsg_max_live_reads_all).  Computed on request and cached until the reads or the barcode table change.  Returns the bound, -1 on
 * error. */
int64_t lsg_max_live_reads(lsg_ctx* ctx);
/* The same bound over EVERY resident read that carries a barcode, whatever its cell type (>= lsg_max_live_reads): what the
 * genotyping pileup of the unsplit BAM can hold at once (HCCVSingleCellGenotype.py:122) — a lower bound on it, since reads without a
 * usable CB tag are dropped at decode and not resident. */
int64_t lsg_max_live_reads_all(lsg_ctx* ctx);
/* The same question per cell type at POSITION resolution: the largest number of reads a pileup buffer can hold when a read is pushed,
 * counting that read (htslib refuses the push iff buffered + 1 > max_depth: a count with max_depth >= this value drops nothing).  The
 * tile-level bounds above over-count where many reads start and end inside one 64-position tile; lsg_pileup_count and the loads ask for
 * this one only when they cannot rule the cap out (a scan over the genome's positions per cell type: ~10 ms at C4).  Cached until the
 * reads or the barcode table change; -1 on error. */
int64_t lsg_max_live_reads_exact(lsg_ctx* ctx);
/* Restrict counting to the genomic region [ (tid_lo,pos_lo), (tid_hi,pos_hi) ) in (tid,pos) order;
 * positions must be multiples of 64.  This is how windows are sharded over GPUs: every rank loads
 * the reads overlapping its region (reads crossing a boundary are loaded by both ranks) and each
 * pileup column is counted by exactly one rank — the analogue of the reference's per-window
 * POS >= START and POS < END test (BaseCellCounter.py:200).  tid_hi == n_contigs, pos_hi == 0
 * means "to the end".  Reset with (0,0,n_contigs,0). */
int lsg_set_region(lsg_ctx* ctx, int32_t tid_lo, int64_t pos_lo, int32_t tid_hi, int64_t pos_hi);
/* The reference's pileup windows (BaseCellCounter.py --bin, default 50000; MakeWindows :81-113 cuts [1, 1 + bin), [1 + bin, ...) per contig
 * and run_interval opens a fresh bam.pileup per window, :185-191).  Result-neutral for the counts except through max_depth: every window's
 * pileup has a buffer of its own, so lsg_pileup_count replays the cap per window, and the loads that follow never let a resident entry
 * cross a window edge (a read dropped in one window may be counted in the next).  window >= 64; default 50000. */
int lsg_set_pileup_window(lsg_ctx* ctx, int32_t window);
/* One pass for a BAM's load AND its first count.  A rule of the reference counts every BAM exactly once
 * (bam.pileup over all windows, BaseCellCounter.py:182-320, after SplitBamCellTypes.py:65-124 routed the reads); when the
 * count's parameters are known while the reads are loaded - they are in every fused rule - the loads that follow
 * (lsg_load_reads, lsg_load_bam, lsg_load_bam_range) count in the same pass that lays the events out per column: the wave that
 * transposes a block of the store adds its events into the per-position counters while it holds them.  Requires the barcode
 * table (lsg_set_barcodes, at most two cell types), every reference and the region to be set before the load; a load for which
 * the pileup's depth cap could fire (lsg_max_live_reads_all() >= max_depth) is made without the count.  The first
 * lsg_pileup_count after the load with EQUAL parameters, the same barcode table and region returns that count's result without
 * another pass; any other call counts over the resident store as always.  params == NULL switches it off (default). */
int lsg_set_count_at_load(lsg_ctx* ctx, const lsg_count_params* params);
/* What the loads that follow keep beside the count they make (lsg_set_count_at_load).  LSG_STORE_KEEP (default): the tile store, the
 * resident form every later count, region, barcode table and genotyping pass works on.  LSG_STORE_SKIP_WHEN_COUNTED: a rule of the
 * reference reads a BAM, counts it once and is done (BaseCellCounter.py:182-320: one bam.pileup per window, nothing is kept) - when the
 * load can make its count in its own pass (the conditions of lsg_set_count_at_load) it counts straight from the caller's events and
 * writes no store: what derives from that count (lsg_fetch_counts, the exports, lsg_call_step1 ...) works as always, lsg_pileup_count
 * with the load's parameters returns it, and everything that needs the store (another count, lsg_genotype_cells) fails with a message
 * until reads are loaded again.  A load that cannot make its count (the depth cap could fire, more than two cell types) builds the
 * store as under LSG_STORE_KEEP.  When the count's read filters are the load's (lsg_set_load_filter with the count's min_mq,
 * flag_exclude and ignore_orphans: every stored read is admitted) and the tiles rule the depth cap out, such a load carries 8-byte keys
 * alone through its scatter and sort instead of 12-byte key + value pairs (store.hip keys_only): the same count, a tenth faster. */
/* The BAM loads that follow (lsg_load_bam, lsg_load_bam_range) keep the reads without a CB tag or with a barcode that is not listed
 * (cb = -1) instead of dropping them at decode time.  Such a read is never counted (SplitBamCellTypes.py:74-90 routes it nowhere), but
 * the per-cell genotyping piles up the UNSPLIT BAM (HCCVSingleCellGenotype.py:121-122): every read that passes that pileup's own
 * filters takes a place in its max_depth buffer, listed or not, and lsg_genotype_cells_grouped replays the buffer over the resident
 * reads.  Default off (the counting rules never see these reads; their events cost memory).  The host decoder's twin is
 * lsio_set_keep_unlisted. */
int lsg_set_keep_unlisted(lsg_ctx* ctx, int32_t on);
/* SplitBamCellTypes' read filters for the BAM loads that follow (lsg_load_bam, lsg_load_bam_range): --max_nM, --max_NH and --n_trim
 * (SplitBamCellTypes.py:92-173, its flags :199-202).  A read whose cleaned CB is listed is checked in the reference's order: nM > max_nm
 * or no nM tag, NH > max_nh or no NH tag, MAPQ < min_mapq; a read with an nM or NH reason is written to no cell type's BAM, so here it is
 * never counted and is kept only as an unlisted read (lsg_set_keep_unlisted); MAPQ alone keeps its meaning (mapq_filtered, the load
 * filter).  A passing read with n_trim > 0 has the qualities of its trim window set to 0 (:129-170): n_trim bases at either end, or at
 * an end whose CIGAR operation is a soft clip of L bases (with more than one operation) L + n_trim, 30 + n_trim for 20 <= L < 30.  The
 * tags: c C s S i I compare as integers, f as a float; a duplicated tag is read at its first occurrence (htslib bam_aux_get, which
 * pysam's opt() calls).  Where the reference raises - an nM / NH tag of another type, a trim window longer than the read, a passing read
 * without qualities when n_trim > 0 - the load fails with an error naming the read.  max_nm / max_nh < 0: that filter is off; (-1, -1,
 * 0) = every filter off (default). */
int lsg_set_split_filters(lsg_ctx* ctx, int32_t max_nm, int32_t max_nh, int32_t n_trim);
/* The filter reasons of the last BAM load, the columns SplitBamCellTypes' report adds behind CB_not_matched (FILTER_dict, :114-116,
 * 181-187): n[r] records and first_ordinal[r] = the smallest record ordinal of the load (-1: none) with reason
 * r = nm * 6 + nh * 2 + mapq, nm and nh in {0 passed, 1 over the limit, 2 tag not found}, mapq in {0, 1}; r = 0 is Pass_reads.  The
 * report's key of r joins the parts with ';' in that order ("nM_not_found;NH;MAPQ"), its columns come in the order in which the file
 * first produced them: by first ordinal.  A range load counts the records of its key range only.  Both arrays hold 18 entries. */
int lsg_get_split_reasons(lsg_ctx* ctx, int64_t* n, int64_t* first_ordinal);
enum { LSG_STORE_KEEP = 0, LSG_STORE_SKIP_WHEN_COUNTED = 1 };
int lsg_set_store_policy(lsg_ctx* ctx, int32_t policy);

/* ---- hot path -------------------------------------------------------------------------------*/
/* Per-cell-type pileup base counting over every covered column of the loaded reads; replaces
 * split_bam's filter (SplitBamCellTypes.py:65-124), run_interval (BaseCellCounter.py:182-320) for
 * all windows, and the gates at :211,:221,:282,:294.  Results stay on the device.
 * n_rows[c] = emitted sites of cell type c; *n_columns = pileup columns with >=1 counted entry,
 * summed over cell types (the "genomic sites" of BASELINE.json's metric). */
int lsg_pileup_count(lsg_ctx* ctx, const lsg_count_params* params, int64_t* n_rows, int64_t* n_columns);
/* Copies cell type ct's rows to the host in genomic order (tid, pos ascending):
 * keys[n] = (tid<<32)|pos0, ref[n] = reference base, counts[n*42].  The resident rows keep 34 of the 42
 * words; BCr[8] is delivered as BC - BCf (what BaseCellCounter.py:271-279 counts: every read is forward or reverse). */
int lsg_fetch_counts(lsg_ctx* ctx, int32_t ct, int64_t* keys, uint8_t* ref, uint32_t* counts, int64_t capacity);

/* Installs per-cell-type count rows (keys[c][i] = (tid<<32)|pos0 strictly ascending, counts[c] =
 * n_rows[c] x 42 words) as if lsg_pileup_count had produced them: the file-level entry of the
 * MergeCounts / BaseCellCalling_step1 rules, whose inputs are BaseCellCounter TSVs
 * (R:SNVCalling.smk:62-156; merge_cell_types_files reads them at MergeBaseCellCounts.py:139-161). */
int lsg_load_counts(lsg_ctx* ctx, int32_t n_celltypes, const int64_t* const* keys, const uint32_t* const* counts,
                    const int64_t* n_rows);

/* Outer join of the per-cell-type rows on (tid,pos) + step-1 arithmetic on every merged site;
 * replaces merge_cell_types_files (MergeBaseCellCounts.py:116-204) and variant_calling_step1
 * (BaseCellCalling.step1.py:19-476).  *n_sites = merged sites, *n_candidates = sites with ALT != ".". */
int lsg_call_step1(lsg_ctx* ctx, const lsg_call_params* params, int64_t* n_sites, int64_t* n_candidates);
/* Copies call records in genomic order; candidates_only != 0 keeps rows with ALT != "." or FILTER != "." */
int lsg_fetch_calls(lsg_ctx* ctx, lsg_call* out, int64_t capacity, int32_t candidates_only, int64_t* n_out);

/* Compacts call records, in genomic order, into a caller-owned DEVICE buffer (e.g. a torch tensor
 * handed to an RCCL all-gather): kind 0 = every site, 1 = rows step 2 keeps (ALT != "." or
 * FILTER != "."), 2 = PASS candidates only (no site filter and a PASS cell type).  dst_device may be
 * NULL to only count; *n_out receives the number of selected rows. */
int lsg_export_calls(lsg_ctx* ctx, int32_t kind, void* dst_device, int64_t capacity, int64_t* n_out);

/* ---- the tables' text, printed on the device -------------------------------------------------------
 * The rows of the reference's three big tables, byte for byte what its writers print:
 *   LSG_TABLE_COUNTS + c  <sample>.<cell type c>.tsv rows       BaseCellCounter.py:300-308 (one row per count row of cell type c)
 *   LSG_TABLE_MERGED      BaseCellCounts.AllCellTypes.tsv rows  MergeBaseCellCounts.py:59-84,116-204 (outer join, "NA" for an absent cell type)
 *   LSG_TABLE_STEP1       calling.step1.tsv rows                BaseCellCalling.step1.py:430-476 (one row per merged site)
 *   LSG_TABLE_STEP1_KEPT  the rows of that table step 2's awk filter keeps (ALT != "." and FILTER != ".", BaseCellCalling.step2.py:23)
 *   LSG_TABLE_STEP2       calling.step2.tsv rows at --min_distance 0 (LongSom's setting): the kept rows,
 *                         FILTER tagged "RNA_editing_db" / "PoN_SR" / "PoN_LR" by the resident position sets (lsg_load_posset; GetExtraFilters,
 *                         BaseCellCalling.step2.py:142-158; a tag replaces a bare "PASS") and then "gnomAD" by the resident allele set
 *                         (lsg_load_alleleset; none loaded: step 2 without a gnomAD source), "NA" cells empty (step2.py's pandas round trip)
 *   LSG_TABLE_STEP3_ROWS  the rows of LSG_TABLE_STEP2 step 3 can keep (made by lsg_step2_summary, not by lsg_format_table)
 *   LSG_TABLE_CELL_LONG   <id>.SingleCellGenotype.tsv rows      CellClustering/SingleCellGenotype.py:181-224,305 (see lsg_cellgeno_count below)
 *   LSG_TABLE_CELL_DP / _ALT / _VAF / _BIN   the rows of <id>.DpMatrix.tsv, AltMatrix, VAFMatrix, BinaryMatrix (SingleCellGenotype.py:351-379)
 *   LSG_TABLE_BNPC_BIN / _VAF   the SNV rows of BnpC_input/<id>.BinaryMatrix.tsv and VAFMatrix.tsv (FormatInputBnpC.py:16-34; see lsg_cellgeno_filter)
 *   LSG_TABLE_FASTQ       the FASTQ records of a BAM for ctat-LR-fusion (FusionCalling/BamToFastq.py:9-42; made by lsg_bam_fastq below,
 *                         not by lsg_format_table)
 *   LSG_TABLE_STEP3_ALL / _PASS   the rows of calling.step3.unfiltered.tsv and calling.step3.tsv (made by lsg_step3_filter below)
 *   LSG_TABLE_GENE_COUNTS the whole of <id>.counts.formated.txt, its header line included: the cell-by-gene read counts inferCNV reads
 *                         (rules featureCount + format_featureCount, rules/CNACalling.smk:29-75; see lsg_gene_counts below)
 * Rows only (the header lines are the caller's), in the reference's order: contigs in Python string order, positions ascending.
 * At 24 M sites these are 17 GB of text: a kernel prints them from the count rows and call records where they lie (two passes:
 * lengths, then bytes), the host only moves bytes.  The merged and step-1 tables need lsg_call_step1 (its merged site list). */
enum lsg_table { LSG_TABLE_COUNTS = 0, LSG_TABLE_MERGED = LSG_MAX_CELLTYPES, LSG_TABLE_STEP1, LSG_TABLE_STEP1_KEPT, LSG_TABLE_STEP2, LSG_TABLE_STEP3_ROWS,
                 LSG_TABLE_CELL_LONG, LSG_TABLE_CELL_DP, LSG_TABLE_CELL_ALT, LSG_TABLE_CELL_VAF, LSG_TABLE_CELL_BIN,
                 LSG_TABLE_BNPC_BIN, LSG_TABLE_BNPC_VAF, LSG_TABLE_FASTQ, LSG_TABLE_SLOTS };
/* Tables added since continue the numbering where enum lsg_table ends, so that none of its values moves - LSG_TABLE_SLOTS, the number
 * of tables its callers were built against, among them.  LSG_TABLE_ALL_SLOTS bounds every table index lsg_format_table,
 * lsg_copy_table, lsg_append_table and lsg_free_table serve. */
enum lsg_table_more { LSG_TABLE_GENE_COUNTS = LSG_TABLE_SLOTS, LSG_TABLE_HCCV2, LSG_TABLE_HCCV3, LSG_TABLE_HCCV_PASS,
                      LSG_TABLE_STEP3_ALL, LSG_TABLE_STEP3_PASS, LSG_TABLE_MORE_SLOTS };
/* ... and the file images lsg_split_bam and lsg_bgzf_compress make (below) continue it again: LSG_TABLE_SPLIT_BAM + t is cell type t's
 * BAM file (t < LSG_MAX_CELLTYPES), LSG_TABLE_BGZF the BGZF file of lsg_bgzf_compress's bytes.  Bytes, not text: whole files, served by
 * lsg_copy_table / lsg_append_table / lsg_free_table like any table, refused by lsg_format_table. */
enum lsg_table_bgzf { LSG_TABLE_SPLIT_BAM = LSG_TABLE_MORE_SLOTS, LSG_TABLE_BGZF = LSG_TABLE_SPLIT_BAM + LSG_MAX_CELLTYPES, LSG_TABLE_BGZF_SLOTS };
/* ... and the .bai files of lsg_split_bam's BAMs (LSG_TABLE_SPLIT_BAI + t, under lsg_set_split_index) and of lsg_bam_index (LSG_TABLE_BAI). */
enum lsg_table_bai { LSG_TABLE_SPLIT_BAI = LSG_TABLE_BGZF_SLOTS, LSG_TABLE_BAI = LSG_TABLE_SPLIT_BAI + LSG_MAX_CELLTYPES, LSG_TABLE_ALL_SLOTS };
/* Names the rows print: contig_names / celltype_names are '\n'-joined, in lsg_set_contigs / cell-type index order. */
int lsg_set_table_names(lsg_ctx* ctx, int32_t n_contigs, const char* contig_names, int32_t n_celltypes, const char* celltype_names);
/* Prints one table into a device buffer the handle keeps for it (until lsg_free_table or the next format of the same table);
 * *n_bytes = size of the text.  The text is a snapshot: later counts and calls do not change it. */
int lsg_format_table(lsg_ctx* ctx, int32_t table, int64_t* n_bytes);
/* The formatted text into host memory (capacity >= its size). */
int lsg_copy_table(lsg_ctx* ctx, int32_t table, char* dst_host, int64_t capacity);
/* Appends the formatted text to the file at `path` (created if absent): device -> pinned staging -> pwrite, pipelined on a stream of
 * its own.  Only reads the table's buffer: may run on another host thread beside any other call on the handle except
 * lsg_format_table / lsg_free_table of the same table and lsg_destroy. */
int lsg_append_table(lsg_ctx* ctx, int32_t table, const char* path);
/* What BaseCellCalling.step3.py needs of the whole step-2 table before it parses anything, read off LSG_TABLE_STEP2's text on the device
 * (directly after its lsg_format_table): kinds[c] = which kinds of cell column c of n_cols holds over ALL rows, as the bits 1 missing
 * value, 2 integer, 4 float, 8 a number pandas would print differently, 16 anything else (pandas infers a column's dtype over the whole
 * file: step3.py:41 reads it all; bits other than 16 mean nothing in a column that has 16); and, as table LSG_TABLE_STEP3_ROWS of
 * *n_survivor_bytes bytes, the rows whose FILTER holds none of the patterns step 3 drops rows by (step3.py:49-52 for chrM rows, :60-84
 * for the others) and whose Cell_types is not "Non-Cancer" - the only rows step 3 has to parse. */
int lsg_step2_summary(lsg_ctx* ctx, int32_t n_cols, uint8_t* kinds, int64_t* n_survivor_bytes);
/* Frees one table's text (table < 0: every table's, and the flat row copies they were printed from). */
int lsg_free_table(lsg_ctx* ctx, int32_t table);

/* ---- the high-confidence cancer variant filter over the step-2 table's text (csrc/hccv.hip, csrc/hccv_core.h) ---------------------
 * HCCV_SNV of CellTypeReannotation/HighConfidenceCancerVariants.py:8-88 with MultiAllelic_filtering (:90-163), DP_filtering (:200-209)
 * and MCF_filtering (:212-255), decided and printed row by row where the table's text lies - the step between the two passes of the
 * cell-type re-annotation, which reads the whole pass-1 step-2 table.  The rows of <out>.HCCV.tsv2 become table LSG_TABLE_HCCV2, those
 * of <out>.HCCV.tsv3 LSG_TABLE_HCCV3 (every non-chrM row in input order, then the chrM rows: pd.concat, :75), the rows of .tsv3 whose
 * verdict is PASS LSG_TABLE_HCCV_PASS (a few hundred: the caller applies the cluster test, :165-197, to them).  Rows only; the header
 * lines are the caller's.  lsg_copy_table / lsg_append_table / lsg_free_table serve the three like any table.
 *   col[]          where the header line has #CHROM Start REF ALT FILTER Cell_types Dp Nc Bc Cc VAF MCF Cancer Non-Cancer, of n_cols <= 64
 *   two_delta_vaf  2 * delta_vaf as the caller's arithmetic gives it (the comparison is the reference's, operation for operation)
 * A row that cannot be decided as pandas and the reference's Python would decide it makes the whole call undecided: info->n_undecided
 * > 0 with the smallest such row's ordinal and its reason, no table is made, and the caller runs the reference's frame code over the
 * whole table.  Nothing is guessed.  info->kinds: as lsg_step2_summary's, filled by lsg_hccv_filter_text only. */
#define LSG_HCCV_COLS 14
enum lsg_hccv_reason { LSG_HCCV_OK = 0,
                       LSG_HCCV_SHORT_ROW,      /* fewer fields than the header has columns */
                       LSG_HCCV_LONG_ROW,       /* more */
                       LSG_HCCV_ODD_TEXT,       /* a quote, a carriage return or a '#' in the row, or an empty line */
                       LSG_HCCV_MISSING,        /* #CHROM, Start, ALT, FILTER or a needed cell-type column is a missing cell */
                       LSG_HCCV_NUMBER,         /* a needed field is not the number it should be (or a division by zero follows from it) */
                       LSG_HCCV_MAX_ZERO,       /* a multi-allelic row without a non-reference read in the cancer column */
                       LSG_HCCV_CELL_TYPES,     /* no cell type, more than two, or two of which neither is Cancer */
                       LSG_HCCV_TOO_LONG,       /* a FILTER of more than 256 bytes to strip */
                       /* lsg_step3_filter's own */
                       LSG_STEP3_CHROM_COLON,   /* a ':' in #CHROM or in the ALT that INDEX takes: INDEX would not split into its three parts */
                       LSG_STEP3_ALT,           /* an ALT whose first character is none of ACTG */
                       LSG_STEP3_INDEX_LONG,    /* a clustered row's INDEX of more than LSG_STEP3_INDEX_MAX bytes */
                       LSG_STEP3_POSITION };    /* a PASS row's Start is no plain integer: the cluster test would raise */
typedef struct {
    int32_t n_cols; int32_t col[LSG_HCCV_COLS];
    int32_t pad_;
    double min_dp, delta_vaf, two_delta_vaf, delta_mcf;
} lsg_hccv_params;
typedef struct {
    int64_t rows_in, rows_tsv2, rows_tsv3, rows_pass;
    int64_t bytes_tsv2, bytes_tsv3, bytes_pass;
    int64_t n_undecided, first_undecided;       /* rows that could not be decided, the smallest ordinal among them (-1: none) */
    int32_t reason;                             /* lsg_hccv_reason of that row */
    float ms_rows, ms_decide, ms_print;         /* HIP-event times: the newline pass and compaction, the decide-and-measure kernel, the print kernel */
    uint8_t kinds[64];
} lsg_hccv_info;
/* Over the resident text of LSG_TABLE_STEP2 (lsg_format_table first; the text and lsg_step2_summary's table are left as they are). */
int lsg_hccv_filter(lsg_ctx* ctx, const lsg_hccv_params* params, lsg_hccv_info* info);
/* Over a table in host memory: the data rows of a step-2 file, leading lines that start with '#' skipped; uploaded through pinned
 * staging, row starts found on the device. */
int lsg_hccv_filter_text(lsg_ctx* ctx, const char* text, int64_t n_bytes, const lsg_hccv_params* params, lsg_hccv_info* info);

/* ---- step 3's final filters over the step-2 table's text (csrc/step3.hip, csrc/step3_core.h) --------------------------------------
 * BaseCellCalling.step3.py:41-316, decided and printed row by row where the text lies: the Cell_types and FILTER drops, MultiAllelic_filtering
 * (:163-231), chrM_filtering (:101-161), BC_CC_filtering (:233-251), BetaBino_filtering (:254-280) and the cluster tag (:283-306).  The
 * rows of calling.step3.unfiltered.tsv become table LSG_TABLE_STEP3_ALL (every non-chrM row in input order, then the chrM rows:
 * pd.concat), the rows whose STEP3FILTER is exactly PASS after the cluster tag LSG_TABLE_STEP3_PASS (calling.step3.tsv).  Rows only;
 * the header lines are the caller's.  lsg_copy_table / lsg_append_table / lsg_free_table serve the two like any table.
 * The cluster test needs a row's neighbours in string-sorted order: the call copies the PASS rows' (ordinal, INDEX) to the host - a few
 * hundred -, sorts and tests them there, and sends the INDEX texts to tag back as sorted records of LSG_STEP3_INDEX_MAX + 1 bytes, which
 * every kept row's lane searches for the INDEX it prints.
 *   col[]   where the header line has #CHROM Start REF ALT FILTER Cell_types Dp Nc Bc Cc VAF MCF Cell_type_Filter Cancer Non-Cancer, of
 *           n_cols <= 64 (Non-Cancer may be -1: a table of one cell type)
 * An undecided row makes the whole call undecided exactly as lsg_hccv_filter's does (the same info fields, enum lsg_hccv_reason), and
 * the caller runs calling.step3 over the same input.  info->kinds: as lsg_step2_summary's, filled by lsg_step3_filter_text only. */
#define LSG_STEP3_COLS 15
#define LSG_STEP3_INDEX_MAX 63
typedef struct {
    int32_t n_cols; int32_t col[LSG_STEP3_COLS];
    double delta_vaf, delta_mcf;
    int64_t min_ac_reads, min_ac_cells, clust_dist;
} lsg_step3_params;
typedef struct {
    int64_t rows_in, rows_all, rows_pass;       /* data rows read, rows of the unfiltered table, rows of the final table */
    int64_t rows_pass_unclustered, n_clustered; /* PASS rows before the cluster tag, INDEX texts the cluster test tags */
    int64_t bytes_all, bytes_pass;
    int64_t n_undecided, first_undecided;       /* rows that could not be decided, the smallest ordinal among them (-1: none) */
    int32_t reason;                             /* lsg_hccv_reason of that row */
    float ms_rows, ms_decide, ms_cluster, ms_print;   /* HIP-event times of the newline pass, the decide kernel and the print kernel; host time of the cluster round trip */
    int32_t pad_;
    uint8_t kinds[64];
} lsg_step3_info;
/* Over the resident rows of LSG_TABLE_STEP3_ROWS as lsg_step2_summary left them (which stay as they are). */
int lsg_step3_filter(lsg_ctx* ctx, const lsg_step3_params* params, lsg_step3_info* info);
/* Over a whole step-2 table in host memory: leading lines that start with '#' skipped, every drop applied. */
int lsg_step3_filter_text(lsg_ctx* ctx, const char* text, int64_t n_bytes, const lsg_step3_params* params, lsg_step3_info* info);

/* ---- FASTQ for the fusion caller, printed on the device (csrc/fastq.hip) ---------------------------
 * A BAM's records as the FASTQ text ctat-LR-fusion reads, into table LSG_TABLE_FASTQ (lsg_copy_table / lsg_append_table / lsg_free_table
 * serve it like any table; all offsets are 64-bit).  Replaces bam_to_fastq (FusionCalling/BamToFastq.py:9-42: pysam iteration,
 * read.to_dict(), four f.write per read) and, in routed mode, the chain of rules/FusionCalling.smk:3-37: the per-cell-type BAMs of
 * SplitBamCellTypes, one BamToFastq per cell type and ConcatFastq.  The front half is lsg_load_bam's (H2D, BGZF inflate + CRC32, record
 * chain, record list); -4 likewise means the record chain did not settle: print that file on the host (lsio_bam_fastq).  The reference
 * table the records are validated against is read from the file's own header (the bytes before first_record_offset), so an unaligned BAM
 * without references works; the call reads and changes nothing of a resident load (store, rows, call records).
 *
 * Every printed record is   @<CB>^<UMI>^<name>\n<seq>\n+\n<qual>\n   with
 *   name  the NUL-terminated read name
 *   seq   "=ACMGRSVTWYHKDBN"[code] per base, "*" when l_seq == 0;  qual  byte + 33 per base, "*" when l_seq == 0 or the first byte is 0xFF
 *         (the SAM text pysam's to_dict() goes through)
 *   CB    the value of the FIRST aux field named CB (bam_aux_get order) without ONE trailing "-1" (re.sub("-1$", ...): "X-2" stays,
 *         "X-1-1" -> "X-1", "-1" -> "")
 *   UMI   the first UB field's value; else, for a name with at least one '.', its second-to-last '.'-separated field without its last
 *         three characters (may be empty); else "NA"
 * A record that cannot be printed ends the call with an error naming its ordinal, and no text is kept: no CB field (LSG_FASTQ_NO_CB:
 * the reference would print the PREVIOUS read's barcode, or raise on the first read - not reproduced), a first CB / UB field that is not
 * of type Z (LSG_FASTQ_CB_TYPE / _UB_TYPE: get_tag(.., "Z")[0] would print one character or raise), and in routed mode with --max_nM /
 * --max_NH set an nM / NH tag that is not a number (LSG_FASTQ_NM_TYPE / _NH_TYPE, as lsg_load_bam refuses it).  info->bad_ordinal /
 * bad_kind name the smallest such ordinal (-1 / LSG_FASTQ_OK: none) also when the call fails for it.
 *
 * Plain mode (barcodes == NULL; celltype_of, n_celltypes, min_mapq unused): every record of the file in file order, unmapped ones
 * included (the script opens with check_sq=False and iterates, it does not fetch()); n_printed[0] / n_bytes[0].
 * Routed mode: barcodes = n_barcodes cleaned strings joined by '\n', celltype_of[i] in [0, n_celltypes) (duplicated strings: the last
 * wins).  A record is printed iff SplitBamCellTypes.py:65-124 writes it to a cell type's BAM - placed on a reference, CB:Z found, its
 * cleaned barcode listed, filter reason 0 under min_mapq and the handle's lsg_set_split_filters limits - decided by the same code as
 * lsg_load_bam's (bamrec_core.h scan_aux / cb_lookup / reason_of).  The text is cell type 0's records in file order, then cell type 1's,
 * ...: n_printed[t] records and n_bytes[t] bytes each.  A record that is routed nowhere cannot be a bad record, with
 * one exception: the nM / NH type of a read whose barcode is listed is reported whatever its MAPQ, because the reference compares the tag
 * (and raises TypeError) before its MAPQ test (SplitBamCellTypes.py:95-108), as lsg_load_bam refuses such a read.  With --n_trim set on the handle
 * (lsg_set_split_filters n_trim > 0) the call refuses: the reference would write qualities of 0 into the split BAMs, and none of
 * LongSom's rules sets it. */
enum { LSG_FASTQ_OK = -1, LSG_FASTQ_NO_CB = 0, LSG_FASTQ_CB_TYPE = 1, LSG_FASTQ_UB_TYPE = 2, LSG_FASTQ_NM_TYPE = 3, LSG_FASTQ_NH_TYPE = 4 };
typedef struct {
    int64_t n_records;
    int64_t n_printed[LSG_MAX_CELLTYPES], n_bytes[LSG_MAX_CELLTYPES];   /* plain mode: index 0 only */
    int64_t bad_ordinal; int32_t bad_kind;                               /* smallest record ordinal that cannot be printed, and why */
    float   ms_h2d, ms_inflate, ms_chain, ms_length, ms_print, ms_total; /* HIP-event times of the phases, wall time of the call */
} lsg_fastq_info;
int lsg_bam_fastq(lsg_ctx* ctx, const uint8_t* file_bytes, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                  const int32_t* celltype_of, int32_t n_celltypes, int32_t min_mapq, lsg_fastq_info* info);

/* ---- SplitBamCellTypes on the device: records routed, BGZF-deflated where they lie (csrc/split.hip) ---------------
 * One BAM file per cell type out of the unsplit BAM's bytes, as tables LSG_TABLE_SPLIT_BAM + t.  Replaces split_bam
 * (SplitBamCellTypes.py:39-192: pysam fetch, read.opt("CB"), the filters, outfile.write through htslib's bgzf + zlib on one thread); the
 * host twin is lsio_split_bam_filtered.  Arguments as lsg_bam_fastq's routed mode; the limits are lsg_set_split_filters', and unlike the
 * FASTQ call --n_trim is honoured.  The front half is lsg_load_bam's; -4 likewise means the record chain did not settle (split that
 * file on the host), -3 that the device has no room for it (the library's out-of-memory code: likewise).  Reads and changes nothing of
 * a resident load.
 *   routed   a record goes to cell type celltype_of[i]'s file iff SplitBamCellTypes.py:65-124 writes it there: placed on a reference
 *            (refID >= 0: infile.fetch()), a CB:Z field found (the FIRST one, as read.opt("CB") and lsio_split_bam_filtered take it; the
 *            loads take the last), its cleaned barcode (up to the first '-') listed, filter reason 0 under min_mapq,
 *            --max_nM and --max_NH - decided by lsg_load_bam's code (bamrec_core.h).  counters / reasons_n / reasons_first are the
 *            report's: total, pass, CB not found, CB not matched, MAPQ; per reason (lsg_get_split_reasons' index) its records and the
 *            smallest record ordinal (-1: none).  Record ordinals count every record of the file.
 *   trim     with n_trim > 0 a written record's qualities inside its trim window are 0 (:129-170), everything else is the input's bytes
 *   files    each file is the input's header (the bytes before first_record_offset; template=infile, :57) and the routed records in file
 *            order, cut into BGZF blocks exactly as htslib's bgzf_write + bgzf_flush_try cut them (and lsio_split_bam_filtered's writer):
 *            the header fills blocks of 0xff00 bytes; a record that does not fit the open block closes it first; a record longer than a
 *            block spills in 0xff00-byte pieces and leaves its tail open.  So every block starts on a record boundary unless a record
 *            is longer than a block, and lsg_load_bam reads the files back without -4.  Every block is one raw DEFLATE stream
 *            (csrc/deflate_core.h: LZ77 + dynamic Huffman codes, literals-only Huffman, or stored - whichever is smallest), its CRC32
 *            and ISIZE; a 28-byte EOF block ends the file.  The compressed bytes differ from zlib's, the inflated ones do not.  An
 *            empty cell type gives a header block + EOF.  The .bai pysam.index writes (:189-192) is not written unless
 *            lsg_set_split_index asks for it (below).
 *   errors   a read on which the reference raises - a trim window longer than the read, no qualities to trim, a non-numeric nM / NH
 *            on a listed barcode under its limit - ends the call with lsio_split_bam_filtered's message behind this call's name; bad_ordinal /
 *            bad_kind (LSG_SPLIT_ERR_*) name the smallest such ordinal, and no table is kept. */
enum { LSG_SPLIT_OK = 0, LSG_SPLIT_ERR_TRIM_LONG = 1, LSG_SPLIT_ERR_NO_QUAL = 2, LSG_SPLIT_ERR_NM_TYPE = 3, LSG_SPLIT_ERR_NH_TYPE = 4 };
typedef struct {
    int64_t n_records;                                             /* records of the file, unplaced ones included */
    int64_t counters[5];                                           /* total, pass, cb_not_found, cb_not_matched, mapq */
    int64_t reasons_n[18], reasons_first[18];
    int64_t n_written[LSG_MAX_CELLTYPES], n_ubytes[LSG_MAX_CELLTYPES];      /* per cell type: records, uncompressed bytes (header included) */
    int64_t n_blocks[LSG_MAX_CELLTYPES], n_file_bytes[LSG_MAX_CELLTYPES];   /* ... BGZF blocks (without the EOF block), the file's bytes */
    int64_t bad_ordinal; int32_t bad_kind;
    int32_t pad_;
    float   ms_h2d, ms_inflate, ms_chain, ms_route, ms_cut, ms_gather, ms_deflate, ms_crc, ms_pack, ms_total;
    /* HIP-event times: the front's three, route + place, gather, deflate, CRC, scan + pack; wall: the cut on the host, the call */
} lsg_split_info;
int lsg_split_bam(lsg_ctx* ctx, const uint8_t* file_bytes, int64_t n_bytes, int64_t first_record_offset, const char* barcodes, int32_t n_barcodes,
                  const int32_t* celltype_of, int32_t n_celltypes, int32_t min_mapq, lsg_split_info* info);
/* n bytes of host memory as one BGZF file (blocks of 0xff00 bytes, the EOF block) into table LSG_TABLE_BGZF; *n_bytes_out its size. */
int lsg_bgzf_compress(lsg_ctx* ctx, const uint8_t* data, int64_t n, int64_t* n_bytes_out);

/* ---- The BAM index on the device: bins, chunks, the linear index, the file's bytes (csrc/bamindex.hip) -----------------------------
 * The .bai of a coordinate-sorted BAM (SAM specification section 5.2) into table LSG_TABLE_BAI: what samtools index / pysam.index write
 * (SplitBamCellTypes.py:189-192; rule IndexBarcodedBam_PoN).  The host twin is lsio_build_bai_full; both write this project's canonical
 * form, byte for byte:
 *   offsets   a record starts at (file offset of the non-empty BGZF block holding the first byte of its block_size word) << 16 | offset
 *             inside it, and ends where the file's next record starts; the last one at (file offset behind the last non-empty block) << 16
 *   interval  [pos, pos + rlen), rlen the reference bases its CIGAR consumes, 1 where that is 0; the flag is not consulted; the bin is
 *             reg2bin of the interval, not the record's own bin field
 *   chunks    per reference every maximal run of file-consecutive records of one bin is a chunk; a bin's chunks in file order, two
 *             neighbours merged when the second starts in the block where the first ends (htslib's adjacent-block merge).  htslib's
 *             roll-up of small bins into their parents is not made
 *   bins      in ascending order; a reference with records ends with the pseudo-bin 37450: (first start, last end), (n_mapped,
 *             n_unmapped by flag 0x4).  A reference without records: n_bin = 0, n_intv = 0
 *   linear    n_intv = the last 16 kb window a record of the reference touches + 1; ioffset[w] = the smallest start of the records
 *             overlapping w, an unset window the value before it, leading ones the reference's first set value (lsio_build_bai's values)
 *   n_no_coor the records with refID < 0
 *   refused   (rc -1, no table, bad_ordinal / bad_kind name the smallest such record ordinal; of several kinds at one record the smallest)
 *             a file that is not coordinate-sorted - (refID, pos) non-decreasing over the placed records, the unplaced ones last;
 *             a placed record with pos < 0; an interval that ends beyond 2^29
 * The front half is lsg_load_bam's; -4 / -3 mean what they mean for lsg_split_bam: index that file on the host.  -3 is also what an
 * index of 2^31 windows or more returns (about 65 536 references of 2^29 each): more than the device builder holds. */
enum { LSG_BAI_OK = 0, LSG_BAI_ERR_UNSORTED = 1, LSG_BAI_ERR_NEG_POS = 2, LSG_BAI_ERR_TOO_FAR = 3 };
typedef struct {
    int64_t n_records, n_placed, n_no_coor;                        /* records of the file, those with refID >= 0, the others */
    int64_t n_runs, n_chunks, n_bins, n_windows;                   /* runs, chunks after the merge, bins (both without the pseudo-bins), windows */
    int64_t n_bytes;                                               /* the .bai file's bytes */
    int64_t bad_ordinal; int32_t bad_kind;                         /* -1 / 0: none */
    int32_t pad_;
    float   ms_h2d, ms_inflate, ms_chain, ms_facts, ms_runs, ms_linear, ms_print, ms_total;
    /* HIP-event times: the front's three (0 for a split's index), the records' facts and checks, runs + sort + chunks, the linear index,
     * scans + print; wall: the call (for a split's index: the part of lsg_split_bam spent on this cell type's index) */
} lsg_bai_info;
int lsg_bam_index(lsg_ctx* ctx, const uint8_t* file_bytes, int64_t n_bytes, int64_t first_record_offset, lsg_bai_info* info);
/* on != 0: lsg_split_bam also leaves the index of every cell type's file - of an empty one too - as table LSG_TABLE_SPLIT_BAI + t, made
 * of the routing's own arrays (the routed records' facts, their offsets in their streams, the block cut, the packed blocks' sizes),
 * not by reading the files again; an input the index refuses (above; ordinals count the records of that cell type's file) then fails
 * the whole call, which keeps neither BAM nor BAI tables.  Off (the default): the call is what it was, and frees the BAI tables of an
 * earlier call.  An index that finds no room on the device ends the call with -3 like any other reserve of it, after the BAMs were made:
 * no table is kept, split and index that file on the host.  lsg_get_split_index_info: cell type t's index of the last lsg_split_bam
 * under the switch; of a call that refused an input, the cell types up to and including the refused one.  -2 when there is none, and
 * then the error text is left as it is: after a failed lsg_split_bam it stays that call's. */
int lsg_set_split_index(lsg_ctx* ctx, int on);
int lsg_get_split_index_info(lsg_ctx* ctx, int t, lsg_bai_info* info);

/* Position sets (RNA-editing / PoN_SR / PoN_LR; build_dict, BaseCellCalling.step2.py:197-221):
 * sorted unique keys (tid<<32)|pos1 resident in HBM; kind in [0,3). */
int lsg_load_posset(lsg_ctx* ctx, int32_t kind, const int64_t* keys, int64_t n, int32_t on_device);
/* Membership of n query keys in set `kind` (GetExtraFilters, step2.py:142-158). hits[i] = 0/1. */
int lsg_probe_posset(lsg_ctx* ctx, int32_t kind, const int64_t* keys, int64_t n, uint8_t* hits, int32_t on_device);

/* Allele set (step 2's gnomAD filter, BaseCellCalling.step2.py:98-114,223-235): the single-base alleles whose population AF is at or
 * above --gnomAD_max, as sorted unique keys
 *     (tid << 48) | (pos1 << 16) | (REF byte << 8) | ALT byte
 * resident in HBM.  pos1 is the 1-based position the tables print, REF and ALT the bytes they print: two keys are equal exactly when the
 * strings the reference looks up are.  Limits: tid < LSG_ALLELE_MAX_TID and pos1 < 2^32 (a run beyond them keeps step 2 on the host).
 * While a set is loaded, LSG_TABLE_STEP2 probes every row whose ALT field is exactly one base (one cell type with candidates, carrying
 * one alternative; "A|C" and "A,A" match nothing in the reference's lookup either) and appends "gnomAD" to the FILTER of a hit, after
 * the position sets' tags (it replaces a bare "PASS").  n = 0 is a valid set (a source is present, nothing hits); n < 0 unloads the
 * set, after which the table is what it is without a gnomAD source. */
#define LSG_ALLELE_MAX_TID 32768
int lsg_load_alleleset(lsg_ctx* ctx, const int64_t* keys, int64_t n, int32_t on_device);
/* Membership of n query keys in the loaded allele set (an error when none is loaded). hits[i] = 0/1. */
int lsg_probe_alleleset(lsg_ctx* ctx, const int64_t* keys, int64_t n, uint8_t* hits, int32_t on_device);
/* The allele keys of the rows step 2 keeps (those of LSG_TABLE_STEP1_KEPT) whose ALT is one base, in the table's row order, into
 * keys_out (host memory, `capacity` keys; NULL to only count): what a gnomAD source has to be asked about for this run.  *n = their
 * number.  Needs lsg_call_step1 and lsg_set_table_names (the row order is the contigs' string order); fails when a contig index or a
 * position is beyond the key's limits. */
int lsg_step2_allele_queries(lsg_ctx* ctx, int64_t* keys_out, int64_t capacity, int64_t* n);

/* ---- per-cell genotyping at target sites ---------------------------------
 * HCCVSingleCellGenotype.py:82-220 (twin: SNVCalling/SingleCellGenotype.py:84-228): for every target
 * site and every barcode of barcodes.tsv
 *   Dp  = pileup entries of that cell at the site whose symbol is one of A,C,T,G,I,D,N (:147-149; 'O'
 *         and 'NA' are not counted) and whose base quality is >= min_bq (pileup min_base_quality, :123),
 *   Alt = those whose symbol equals the site's expected alt (:171-175).
 * alt_only != 0 is --alt_flag Alt (:150-151): only reads carrying the expected alt are looked at.
 * Read admission: pileup's flag filter and ignore_orphans, min_mq (:123), not secondary / duplicate /
 * supplementary (:168), CB present and listed (:160-164); strict_cb != 0 also drops reads whose raw CB
 * tag carried a "-suffix" (the reference looks the raw tag up in the cleaned table, :160-161;
 * liblongsom_io marks such reads with LSG_FLAG_CB_SUFFIX in read_flag).
 * site_keys = (tid << 32) | pos0, strictly ascending; alt_sym = symbol class 0..6 per site (255 = none).
 * dp / alt: [n_sites][n_cb] uint32, zeroed by the call.  Needs contigs, barcodes and reads. */
#define LSG_FLAG_CB_SUFFIX 0x8000u
typedef struct {
    int32_t  min_bq, min_mq;
    uint32_t flag_exclude;      /* 0xF04 */
    int32_t  ignore_orphans;
    int32_t  alt_only;
    int32_t  strict_cb;
} lsg_genotype_params;
int lsg_genotype_cells(lsg_ctx* ctx, const lsg_genotype_params* params, int64_t n_sites, const int64_t* site_keys,
                       const uint8_t* alt_sym, uint32_t* dp, uint32_t* alt, int32_t on_device);
/* The same with the pileup's depth cap (HCCVSingleCellGenotype.py:122: bam.pileup(CHROM, START, END, ..., max_depth = 200000), one call
 * per window of target sites, build_dict_variants :245-265): the sites [group_off[g], group_off[g + 1]) are one such window (same
 * contig), its region [first site - 1, last site + 1).  For every window whose region can hold more than max_depth reads, htslib's rule
 * (a read that is not the first of its start position is dropped while the buffer exceeds max_depth; lsg_count_params.max_depth states
 * it) is replayed over the resident reads that overlap the region and the reads it drops are left out of that window's sites.  The
 * stream is the reads of the resident load — all cell types, reads with a listed barcode (the decoders keep no others): for a BAM
 * whose reads all carry listed barcodes this is the reference's buffer, otherwise a lower bound on it.  max_depth <= 0 or n_groups == 0:
 * lsg_genotype_cells.  Free while lsg_max_live_reads_all() stays below the cap. */
int lsg_genotype_cells_grouped(lsg_ctx* ctx, const lsg_genotype_params* params, int32_t max_depth, int64_t n_sites, const int64_t* site_keys,
                               const uint8_t* alt_sym, int64_t n_groups, const int64_t* group_off, uint32_t* dp, uint32_t* alt, int32_t on_device);
/* round(betabinom.sf(k - 0.001, n, alpha, beta), 4) * 1e4 for n_items integer (k, n) pairs, evaluated on the
 * device with the step-1 tail code (HCCVSingleCellGenotype.py:204; k[i] <= 0 gives 10000). */
int lsg_betabinom_sf4(lsg_ctx* ctx, int64_t n_items, const uint32_t* k, const uint32_t* n, double alpha, double beta, int32_t* out_p4);
/* The same tails with the UNROUNDED fp64 value beside the rounded one: what the exactness audit measures (how far every p of a
 * workload lies from a 4-decimal rounding tie of round(betabinom.sf(...), 4), BaseCellCalling.step1.py:196,201; tools/p_margins.py). */
int lsg_betabinom_sf(lsg_ctx* ctx, int64_t n_items, const uint32_t* k, const uint32_t* n, double alpha, double beta, int32_t* out_p4, double* out_p);

/* ---- per-cell verdicts and cell-by-variant matrices -----------------------
 * CellClustering/SingleCellGenotype.py (rule SingleCellGenotype, rules/CellClustering.smk:4-103): the twin of the script above re-piled at
 * the final SNVs, with a verdict per cell and four matrices.  lsg_cellgeno_count counts Dp / Alt as lsg_genotype_cells_grouped does
 * (run_interval, :84-178; this script cleans the CB tag before the lookup, :164-169: strict_cb = 0) and, with the counts where they lie,
 * gives every (site, barcode) cell (:181-218)
 *   vaf4    round(ALT / DP, 4) * 1e4 (:194), -1 where DP = 0 (the script prints ".")
 *   p4      round(betabinom.sf(ALT - 0.001, DP, alpha2, beta2), 4) * 1e4 (:204), -1 where the script prints "." (DP = 0, ALT = 0, or a
 *           site flagged in is_chrm: --chrM_contaminant True and a contig named exactly chrM, :197)
 *   status  LSG_CELL_NOCOVERAGE (DP = 0), _NOALT (ALT = 0), _LOWVAF_CHRM (flagged site, VAF < 0.3 i.e. vaf4 < 3000), _BETABIN_PROBLEM
 *           (p4 / 10000.0 >= pvalue), _PASS (:192-211)
 *   bin     BinMutationStatus: 1 PASS, 3 NoCoverage, 0 otherwise (:213-218)
 * and every barcode the number of sites with DP > 0 (n_covered) and with PASS (n_pass).  The arrays [n_sites][n_cb] stay on the device
 * until the next lsg_cellgeno_count / lsg_cellgeno_load_counts; lsg_cellgeno_fetch copies them out (any pointer may be NULL).
 * lsg_cellgeno_load_counts classifies Dp / Alt tables the caller brings (counts summed over ranks, test grids) instead of counting. */
enum { LSG_CELL_NOCOVERAGE = 0, LSG_CELL_NOALT, LSG_CELL_LOWVAF_CHRM, LSG_CELL_BETABIN_PROBLEM, LSG_CELL_PASS };
int lsg_cellgeno_count(lsg_ctx* ctx, const lsg_genotype_params* params, int32_t max_depth, int64_t n_sites, const int64_t* site_keys,
                       const uint8_t* alt_sym, const uint8_t* is_chrm, int64_t n_groups, const int64_t* group_off,
                       double alpha2, double beta2, double pvalue);
int lsg_cellgeno_load_counts(lsg_ctx* ctx, int64_t n_sites, int32_t n_cb, const uint32_t* dp, const uint32_t* alt, const uint8_t* is_chrm,
                             double alpha2, double beta2, double pvalue);
int lsg_cellgeno_fetch(lsg_ctx* ctx, uint32_t* dp, uint32_t* alt, int32_t* vaf4, int32_t* p4, uint8_t* status, uint8_t* bin,
                       int64_t* n_covered, int64_t* n_pass);
/* The strings and orders the five tables print (uploaded once; string i of a blob = blob[off[i] .. off[i + 1])):
 *   head   per site: "#CHROM .. Num_cells_expected", the first seven columns joined by tabs (:222)
 *   index  per site: INDEX = CHROM:POS:ALT_expected up to its first comma (:221)
 *   label  per site: the matrices' first column (INDEX after sort_chr_index, :342-348)
 *   cb, ct per barcode: CB and Cell_type_observed
 *   long_order   the sites in the long table's order (windows by chromosome text and smallest position, :309-317; a site appears once)
 *   mat_order    the sites in the matrices' row order (natsorted INDEX with chrM last, :342-345)
 *   col_src      per matrix column (distinct CB, sorted as pandas' pivot sorts them): its barcode, or -1 for a barcode only the fusion
 *                file names - an empty cell;  float_cells != 0: the integer matrices print "3.0" (pandas, a pivot with gaps)
 * lsg_format_table(LSG_TABLE_CELL_LONG) then prints n_long x n_cb rows of 16 columns, LSG_TABLE_CELL_DP .. _BIN one row per site of
 * mat_order: label, then n_cols cells.  Header lines and the fusion rows (a handful) are the caller's. */
typedef struct {
    const char* head;  const uint32_t* head_off;
    const char* index; const uint32_t* index_off;
    const char* label; const uint32_t* label_off;
    const char* cb;    const uint32_t* cb_off;
    const char* ct;    const uint32_t* ct_off;
    int64_t n_long; const int32_t* long_order;
    int64_t n_mat;  const int32_t* mat_order;
    int32_t n_cols; int32_t float_cells; const int32_t* col_src;
} lsg_cellgeno_text;
int lsg_cellgeno_set_text(lsg_ctx* ctx, const lsg_cellgeno_text* text);

/* ---- BnpC's input from the resident cells (CellClustering/FormatInputBnpC.py:6-35, rule FormatInputBnpC, rules/CellClustering.smk:105-133)
 * The script reads BinaryMatrix and VAFMatrix back with 3 and "." as NA (:7-8) and filters them.  lsg_cellgeno_filter does so where the
 * cells lie, over the rows of mat_order and the columns of col_src (lsg_cellgeno_set_text first):
 *   a row is kept iff the number of its cells with bin == 1, over the columns with col_src >= 0, is > min_cells_per_mut   (:16)
 *   a column is kept iff the number of its cells with bin != 3 over the KEPT rows is > min_pos_cov; col_src == -1 counts 0  (:19)
 *   a column prints as integers iff col_int_ok[col] != 0 (the caller's half: no float text and no gap in the matrix the script would
 *   have read, fusion rows included) and it is covered at all n_mat rows - pandas gives a column with an NA the dtype float64 (:7)
 * A negative threshold keeps everything.  The fusion rows (labels with "--", :11-13,27) are never filtered by row and never counted:
 * they are the caller's.  lsg_format_table(LSG_TABLE_BNPC_BIN / _VAF) then prints the kept rows over the kept columns, both in input
 * order (:21-27,33-34): label, then per column a tab and nothing for an NA, else "0" / "1" (".0" appended unless the column is
 * integer) resp. repr(vaf4 / 1e4).  lsg_cellgeno_filter_fetch copies out, per row of mat_order, row_keep and row_mut (its count of 1s)
 * and, per column, col_keep, col_cov_kept, col_cov_all (covered cells over the kept / over all rows) and col_int; any pointer may be NULL.
 * A new count, load or lsg_cellgeno_set_text invalidates the filter and both tables. */
int lsg_cellgeno_filter(lsg_ctx* ctx, int32_t min_cells_per_mut, int32_t min_pos_cov, const uint8_t* col_int_ok, int64_t* n_rows_kept, int32_t* n_cols_kept);
int lsg_cellgeno_filter_fetch(lsg_ctx* ctx, uint8_t* row_keep, uint8_t* col_keep, int32_t* row_mut, int32_t* col_cov_kept, int32_t* col_cov_all, uint8_t* col_int);
/* The cells of matrices that were parsed from files: bin [n_sites][n_cb] in {0, 1, 3}, vaf4 = VAF * 1e4 or -1 for NA.  They become the
 * resident bin / vaf4, with status LSG_CELL_NOCOVERAGE where bin == 3 (LSG_CELL_PASS where 1, LSG_CELL_NOALT where 0).  The state holds
 * no counts and no tails: LSG_TABLE_CELL_LONG, _DP and _ALT and the dp / alt / p4 of lsg_cellgeno_fetch are refused until the next count. */
int lsg_cellgeno_load_cells(lsg_ctx* ctx, int64_t n_sites, int32_t n_cb, const uint8_t* bin, const int32_t* vaf4);

/* ---- BnpC's posterior estimate (CellClustering/libs/utils.py:90-245; rule BnpC_clustering, rules/CellClustering.smk:135-176) ----------
 * The deterministic half of BnpC: from the chains' posterior samples to one clustering and its genotypes.  The sampler (libs/CRP.py,
 * libs/MCMC.py) stays the caller's and feeds it.  Nothing else need be resident: no reads, contigs or barcodes.
 * lsg_bnpc_load_samples makes the samples resident: the chains concatenated after burn-in (_concat_chain_results, :206-223).
 *   assign [n_samples][n_cells]   cell i's cluster label in sample s, any integer in [0, n_cells); kept as 16 bits
 *   params [n_samples][k_max][n_muts]   row r = the parameters of the r-th smallest label present in the sample, zero beyond the sample's
 *            cluster count (Chain.update_results, MCMC.py:260-282).  May be NULL: lsg_bnpc_mean_params is then refused.
 * Refused with a message: n_cells < 2 or > 65535, n_samples < 1, a label outside [0, n_cells).  A second load replaces the first.
 * lsg_bnpc_codist counts, for every pair i < j in pdist's condensed order (0,1), (0,2), .., (n-2,n-1), the samples in which the two
 * cells' labels differ: get_dist (:90-97) before its division by n_samples.  The counts stay resident; lsg_bnpc_fetch_dist copies the
 * n (n - 1) / 2 of them out.
 * lsg_bnpc_mpear makes one pass over them for n_cuts candidate clusterings labels [n_cuts][n_cells] (values in [0, n_cells)):
 *   same_pairs[k] = the pairs whose two labels in cut k are equal          (_calc_MPEAR's I.sum(), :134-136)
 *   same_sim[k]   = the sum of n_samples - D over those pairs              (n_samples x (I * pi).sum(), :138)
 *   *dist_sum     = the sum of D over all pairs                            (pi.sum() = (pairs x n_samples - dist_sum) / n_samples, :137)
 * exact integers, whatever the order they were added in; the caller forms the score (:140-143) from them in fp64.
 * lsg_bnpc_mean_params is get_mean_hierarchy_assignment (:149-189) for a final assignment final_assign [n_cells]; its clusters are the
 * n_clusters distinct values, ascending.  Per cluster c and sample s: "same" = all of c's cells carry one label L (:157-162; always for a
 * one-cell cluster), "no others" = L occurs in no cell outside c (:164-167), rel = the distinct labels of the sample smaller than L (the row
 * :178-180 pick).  The samples used are those with both, if any, else those with "same" (:170-175): params[c][m] = the sum of
 * params[s][rel][m], widened to double and added in ascending sample order, divided by their number n_used[c].  Where no sample has
 * "same" (:183-189): the sum over all samples and all of c's cells of the row of the cell's label, divided by n_samples x cells.
 *   params [n_clusters][n_muts] doubles; branch[c] = 0 both criteria, 1 the first only, 2 neither, 3 a one-cell cluster; branch and
 *   n_used may be NULL.
 * lsg_bnpc_linkage: scipy's linkage(D / n_samples, "ward") over the resident counts, every bit of its four columns: the nearest-neighbour
 *            chain walked by one workgroup over a square fp64 working copy (n_cells^2 x 8 bytes of device memory: refused with the byte
 *            count where that is not free), the merges sorted stably by height and named by scipy's union-find on the host.  The tree
 *            stays resident for lsg_bnpc_cut_tree; Z [n_cells - 1][4] may be NULL.
 * lsg_bnpc_cut_tree: scipy's cut_tree(Z, n_clusters) of that tree (made first where lsg_bnpc_linkage was not called since the last
 *            lsg_bnpc_codist), one row of labels per requested cluster number: nodes applied in ascending height, equal heights in
 *            cut_tree's own order, a cluster's label its rank by its lowest cell.  Refused: n_cuts < 1, an n_clusters outside
 *            1 .. n_cells - 1 (scipy answers n_cells itself with zeros).
 * lsg_bnpc_cluster_counts: per sample the labels that more than two cells carry, summed over the samples (utils.py:106-111 before its mean:
 *            *sum_over_samples / n_samples in fp64 is np.mean of the counts).  Needs lsg_bnpc_load_samples alone.
 * lsg_bnpc_unload frees all of it. */
int lsg_bnpc_load_samples(lsg_ctx* ctx, int64_t n_samples, int32_t n_cells, const int32_t* assign, int32_t k_max, int32_t n_muts, const float* params);
int lsg_bnpc_codist(lsg_ctx* ctx);
int lsg_bnpc_fetch_dist(lsg_ctx* ctx, uint32_t* dist, int64_t capacity);
int lsg_bnpc_mpear(lsg_ctx* ctx, int32_t n_cuts, const int32_t* labels, uint64_t* same_pairs, uint64_t* same_sim, uint64_t* dist_sum);
int lsg_bnpc_mean_params(lsg_ctx* ctx, const int32_t* final_assign, int32_t n_clusters, double* params, uint8_t* branch, int32_t* n_used);
int lsg_bnpc_linkage(lsg_ctx* ctx, double* Z);
int lsg_bnpc_cut_tree(lsg_ctx* ctx, int32_t n_cuts, const int32_t* n_clusters, int32_t* labels);
int lsg_bnpc_cluster_counts(lsg_ctx* ctx, int64_t* sum_over_samples);
int lsg_bnpc_unload(lsg_ctx* ctx);

/* ---- BnpC's sampler (CellClustering/libs/CRP.py:17-820, libs/CRP_learning_errors.py, libs/MCMC.py:200-388) ------------------------------
 * Gibbs assignment sweeps, the split-merge move, the Escobar-West concentration update, the parameter Metropolis-Hastings and the
 * error-rate updates, all chains of a run in every kernel.  The random stream (Philox4x32-10 keyed by the chain's seed), the
 * variates and the order of a step are stated in longsom_amd/bnpc_sampler.py, whose numpy twin these calls are held to.
 * lsg_bnpcs_create makes the data and the chains' buffers resident (a second create replaces the first):
 *   one, zero [n_cells][ceil(n_muts / 64)]   the cells' masks: bit m % 64 of word m / 64 is set where the cell shows 1 resp. 0; neither: missing
 *   cfg [10]   FN, FP, the parameter prior's p and q, DP_a_gamma's two numbers, the concentration update's probability, the new cluster's
 *              two log terms (get_lpost_single_new_cluster: per 1 and per 0 of the cell), betaln(p, q)
 *   seeds [n_chains]; n_steps: the run's steps (n_steps + 1 records, step 0 is the start); arena_rows: parameter rows of n_muts floats
 *   per chain held between two fetches.  Refused: n_cells < 2 or > 65535 (the estimate keeps 16-bit labels).
 * lsg_bnpcs_set_state / _get_state move one chain's state: labels [n_cells] in [0, n_cells), theta [n_cells][n_muts] float32 (row = cluster
 * id, rows of free ids are not read) and the concentration.  They are how the start is loaded, and what a move made outside works on.
 * lsg_bnpcs_run makes steps first_step .. first_step + n_steps - 1 (first_step must be the next step; step 0 only records) and records each:
 * ML, the CRP prior's sum over the clusters, the beta prior's log density of their parameters, the cluster count, the concentration, the
 * labels, and from step burn_in on the live clusters' parameter rows in ascending id into the arena.  When a step's rows do not fit the
 * arena the call returns with *done = the steps recorded; lsg_bnpcs_fetch empties the arena and the next call goes on at that step.
 * lsg_bnpcs_fetch copies out labels [n_chains][n_steps + 1][n_cells], scalars [n_chains][n_steps + 1][5] (in the order above), the arena
 * [n_chains][arena_rows][n_muts] (per chain the first arena_used[chain] rows: the kept steps since the last fetch, one after the other) and
 * errors [n_chains]: gamma variates that ran out of their 64 tries.
 * lsg_bnpcs_set_split_merge, called after lsg_bnpcs_create (without it the probability is 0 and no step is a move): every chain takes the
 * non-conjugate split-merge move (CRP.py:417-820) in place of the sweep with probability prob per step, a split with ratio_split and a merge
 * with ratio_merge where both are possible, after `scans` restricted Gibbs scans (run_BnpC.py's -smp, -smr, -sms).  Refused: prob outside
 * [0, 1], ratios that are not positive or do not sum to 1, scans < 0 or > 2^20.
 * lsg_bnpcs_fetch_moves copies out moves [n_chains][n_steps + 1]: what each step so far did: 0 a sweep (and step 0), 1 / 2 a split declined /
 * accepted, 3 / 4 a merge declined / accepted.
 * lsg_bnpcs_set_error_learning, called after lsg_bnpcs_create (without it the rates stay cfg's): every chain has error rates of its own,
 * which start at the priors' means fp_mean, fn_mean (CRP_errors_learning.__init__, CRP_learning_errors.py:18-32), and after a step's
 * parameter move makes with probability prob a Metropolis-Hastings update of FP and then of FN (update_error_rates / MH_error_rates,
 * :52-111; Chain.do_step, MCMC.py:339-342; run_BnpC.py's -eup, -FP_m, -FP_sd, -FN_m, -FN_sd).  Refused: prob outside [0, 1], a mean or an
 * sd outside (0, 1).
 * lsg_bnpcs_set_error_rates loads one chain's rates (the model's FP and FN, CRP.py:36-37), for states written as data.  Refused: a rate
 * outside (0, 1).
 * lsg_bnpcs_fetch_error_rates copies out rates [n_chains][n_steps + 1][2]: FP and FN as each step so far recorded them
 * (Chain.update_results, MCMC.py:256-257), and counts [n_chains][4]: the FP moves accepted and declined, the FN moves accepted and
 * declined (Chain.MH_counter[3], [4], MCMC.py:340-342).
 * lsg_bnpcs_set_fixed_assignment: with on != 0 a step makes neither the sweep, nor the split-merge move, nor the concentration update
 * (Chain.do_step with fix_assign, MCMC.py:321-333): the labels stay the loaded ones; the parameter move, the error update and the record
 * run as always.
 * lsg_bnpcs_extend makes room for add_steps more recorded steps: the run's n_steps grows by add_steps.  Every chain's state, the records
 * made so far, the arena and its fill, the moves' and the rates' counts and the next step stay; the layouts of lsg_bnpcs_fetch, _fetch_moves
 * and _fetch_error_rates hold for the new n_steps.  A chain's stream is a function of (seed, step, purpose), so an extended chain is the
 * chain a create with the larger n_steps would have made.  Refused: before a create, add_steps < 1, and a step count that lsg_bnpcs_create
 * would refuse for its size (the message names the steps it would reach); then, and when the device has no room, the run stays as it was.
 * lsg_bnpcs_psrf: what the lugsail batch-means PSRF (utils.get_lugsail_batch_means_est, utils.py:427-467) needs of every chain's ML
 * records first[chain] .. last - 1, stats [n_chains][5]: their number n, their mean, their sample variance (ddof 1), tau(b) and tau(b / 3)
 * with b = int(n ** 0.5) and tau(b) = b / (a - 1) sum (batch mean - mean)^2 over the a = n / b whole batches of b (get_tau_lugsail,
 * :464-467); both are 0 where n < 9.  The sums are of ML - ML[first], in two passes, in double.  Nothing but stats is moved to the host.
 * Refused: last past the records made, first[chain] < 0 or > last. */
int lsg_bnpcs_extend(lsg_ctx* ctx, int32_t add_steps);
int lsg_bnpcs_psrf(lsg_ctx* ctx, const int32_t* first, int32_t last, double* stats);
int lsg_bnpcs_create(lsg_ctx* ctx, int32_t n_cells, int32_t n_muts, int32_t n_chains, int32_t n_steps, const uint64_t* one, const uint64_t* zero, const double* cfg,
                     const uint64_t* seeds, int64_t arena_rows);
int lsg_bnpcs_set_state(lsg_ctx* ctx, int32_t chain, const int32_t* labels, const float* theta, double dp_alpha);
int lsg_bnpcs_get_state(lsg_ctx* ctx, int32_t chain, int32_t* labels, float* theta, double* dp_alpha);
int lsg_bnpcs_run(lsg_ctx* ctx, int32_t first_step, int32_t n_steps, int32_t burn_in, int32_t* done);
int lsg_bnpcs_fetch(lsg_ctx* ctx, int32_t* labels, double* scalars, float* arena, int64_t* arena_used, int32_t* errors);
int lsg_bnpcs_set_split_merge(lsg_ctx* ctx, double prob, double ratio_split, double ratio_merge, int32_t scans);
int lsg_bnpcs_fetch_moves(lsg_ctx* ctx, int8_t* moves);
int lsg_bnpcs_set_error_learning(lsg_ctx* ctx, double prob, double fp_mean, double fp_sd, double fn_mean, double fn_sd);
int lsg_bnpcs_set_error_rates(lsg_ctx* ctx, int32_t chain, double fp, double fn);
int lsg_bnpcs_fetch_error_rates(lsg_ctx* ctx, double* rates, int32_t* counts);
int lsg_bnpcs_set_fixed_assignment(lsg_ctx* ctx, int32_t on);
int lsg_bnpcs_destroy(lsg_ctx* ctx);

/* ---- the beta-binomial fit of the panel-of-normals branch (scripts/PoN/BetaBinEstimation.py) ---------------------------------------
 * The alpha / beta of the step-1 calls, fitted from the resident count rows instead of by VGAM.  Per row: Alt_CC / Alt_BC = the sum of
 * CC / BC over the alleles a table prints (A C T G I D; N and O are not printed and never reach the reference's sums) that are not REF, Ref_CC = NC - Alt_CC, Ref_BC = DP - Alt_BC; a row is kept iff
 * Alt_CC / (double)NC < 0.10 and Alt_BC / (double)DP < 0.15 (:101-104).  The data of both fits are six value histograms, in this order:
 * Alt_CC, Ref_CC, NC (the cell counts' fit: alpha1, beta1), Alt_BC, Ref_BC, DP (the base counts' fit: alpha2, beta2).  The arithmetic,
 * the start, the step and the stop of the solve are stated in longsom_amd/bbfit.py, whose numpy twin these calls are held to.
 * lsg_bbfit_reset zeroes the six histograms of `capacity` bins each (uint64 [6][capacity]).
 * lsg_bbfit_accumulate makes one pass over the resident count rows of cell type ct - those lsg_pileup_count left or those
 *   lsg_load_counts installed - and adds the kept rows' values.  REF is the loaded reference at the row's site, or, with ref_or_null
 *   given, ref_or_null[r] for row r of the cell type in genomic order (a table's own REF column: no reference need be loaded).
 *   sample_n > 0 thins a table of more than sample_n rows before the filter: row r of table `table` stays iff the uniform of
 *   Philox4x32-10 under key `seed` and counters (table, r low, r high, 0) is below sample_n / rows.  n_rows_seen: the rows the thinning
 *   left; n_rows_kept: those of them the filter kept (either may be NULL).  Errors, after which the histograms must be reset: a value
 *   >= capacity (the message names it - no site is left out silently), a row with DP or NC zero (the reference divides by them).
 * lsg_bbfit_fetch copies the histograms out, lsg_bbfit_add adds foreign ones (same capacity) in: the ranks' exchange.
 * lsg_bbfit_solve: est = alpha1, beta1, alpha2, beta2; one workgroup per fit, every sum in a fixed order: the same histograms give the
 *   same bits on every run.  max_iter 0 means 100.  A fit without rows gives NaN and LSG_BBFIT_NO_DATA. */
enum { LSG_BBFIT_CONVERGED = 0, LSG_BBFIT_ITERATION_CAP = 1, LSG_BBFIT_NO_DATA = 2, LSG_BBFIT_NO_FINITE_MAXIMUM = 3 };
typedef struct {
    int32_t iterations[2];      /* per fit (0 the cell counts', 1 the base counts'): Newton iterations made */
    int32_t status[2];          /* LSG_BBFIT_*; NO_FINITE_MAXIMUM: the iterate left [1e-8, 1e8] (all alternative counts zero, or under-dispersed data) */
    double last_step[2];        /* the larger component of the last step in (log alpha, log beta) */
    double grad_norm[2];        /* norm of the gradient in the log-parameters where that step was made */
} lsg_bbfit_info;
int lsg_bbfit_reset(lsg_ctx* ctx, int64_t capacity);
int lsg_bbfit_accumulate(lsg_ctx* ctx, int32_t ct, const uint8_t* ref_or_null, int32_t table, int64_t sample_n, uint64_t seed, int64_t* n_rows_seen, int64_t* n_rows_kept);
int lsg_bbfit_fetch(lsg_ctx* ctx, uint64_t* hist);
int lsg_bbfit_add(lsg_ctx* ctx, const uint64_t* hist);
int lsg_bbfit_solve(lsg_ctx* ctx, double* est, lsg_bbfit_info* info, int32_t max_iter);

/* ---- cell-by-gene read counts: the expression matrix of the CNA branch ------------------------------------------------------------
 * Replaces rules split_per_bc, featureCount and format_featureCount of workflow/rules/CNACalling.smk:11-75 - one BAM per barcode,
 * `featureCounts -L -a <gtf>` over all of them, a pandas step that names and sums the rows - by one pass over the reads a load left
 * resident.  What is counted (longsom_amd/genecounts.py states it in numpy): the annotation's exons by gene_id,
 * unstranded (featureCounts -t exon -g gene_id -s 0); a read's blocks are its segments; a read with a listed barcode is CONSIDERED
 * when flag & flag_exclude == 0 and mapq >= min_mapq, else tallied Filtered; a considered read is Assigned to the one gene whose
 * exons its blocks overlap by a base or more, NoFeatures without any, Ambiguity with two or more (no -O).  NH is not resident: the
 * multi-mapping rule of featureCounts without -M is not modelled (lsg_set_split_filters' max_NH is what a BAM load offers). */

/* The flattened annotation (stands in for featureCounts' reading of `-a <gtf>`, CNACalling.smk:42-44): n_intervals sorted, disjoint
 * elementary intervals [key, key + len) with key = tid << 32 | start0 (0-based) and start0 + len <= 2^32, label = the index of the
 * one gene covering it or LSG_GENE_AMBIG; row_of_gene[g] in [0, n_rows) = the matrix row gene g adds to (several genes may share a
 * row: format_featureCount's groupby('Geneid').sum(), CNACalling.smk:71) or -1 for a gene that is assigned but printed nowhere (a
 * gene id without a name, :69-70).  Every index a kernel follows is checked here.  Drops a matrix counted under another annotation. */
#define LSG_GENE_AMBIG 0xFFFFFFFEu
int lsg_load_annotation(lsg_ctx* ctx, int64_t n_intervals, const uint64_t* keys, const uint32_t* lens, const uint32_t* labels, int32_t n_genes,
                        const int32_t* row_of_gene, int32_t n_rows);
/* The read filters of a count: featureCounts' -Q (min_mapq, default 0) and the SAM flag bits that remove a record (0x4 = featureCounts
 * without --primary: secondary and supplementary records count, each on its own; | 0x900 = --primary).  CNACalling.smk:41-44 sets none. */
typedef struct { int32_t min_mapq; uint32_t flag_exclude; } lsg_gene_count_params;
/* Of one lsg_gene_counts call: the reads and segments it looked at, its reads per outcome (unlisted: no listed barcode, tallied
 * nowhere), and the HIP-event times of its phases: the segment kernel (interval lookup + fold), the read kernel (matrix and tallies). */
typedef struct {
    int64_t n_reads, n_segs;
    int64_t n_assigned, n_no_features, n_ambiguity, n_filtered, n_unlisted;
    float   ms_segments, ms_reads, ms_total;
    int32_t pad_;
} lsg_gene_count_info;
/* Counts the resident load (stands in for rule featureCount's run, CNACalling.smk:29-44) and ADDS it to the resident matrix (uint32
 * [n_rows][n_cb], barcodes in dense-id order) and tallies (uint64 [n_cb][4]: Assigned, NoFeatures, Ambiguity, Filtered): a second load
 * of more reads of the same sample accumulates, as lsg_bbfit_accumulate does.  Refused with an error code when no annotation is
 * loaded, no reads are resident, or the barcode count differs from the one the matrix was started with; a cell that would pass
 * 2^32 - 1 fails the call.  Reads and changes nothing of the store, the count rows or the calls; lsg_unload_reads leaves the matrix. */
int lsg_gene_counts(lsg_ctx* ctx, const lsg_gene_count_params* params, lsg_gene_count_info* info);
/* The matrix (n_rows x n_cb uint32) and the tallies (n_cb x 4 uint64) to the host; either may be NULL.  What rule featureCount
 * writes as <id>.counts.txt and <id>.counts.txt.summary (CNACalling.smk:34), after format_featureCount's row sums. */
int lsg_gene_counts_fetch(lsg_ctx* ctx, uint32_t* matrix, uint64_t* tallies);
/* The strings LSG_TABLE_GENE_COUNTS prints (stands in for DataFrame.to_csv in format_featureCount, CNACalling.smk:72): the row names
 * (blob + n_rows + 1 offsets; the caller sorts and vets them), the columns as dense barcode ids in output order with their strings
 * (blob + n_cols + 1 offsets, in column order) and the separator byte (',' as the rule writes, '\t' as infercnv.R:14 reads).
 * lsg_format_table(LSG_TABLE_GENE_COUNTS) then prints "Geneid<sep><bc>...\n" and one "<name><sep><count>...\n" per row. */
int lsg_gene_counts_set_text(lsg_ctx* ctx, const char* row_names, const uint32_t* row_off, int32_t n_cols, const int32_t* col_src,
                             const char* col_names, const uint32_t* col_off, int32_t separator);
/* Frees the annotation, the matrix, the tallies, the strings and the table's text (the per-barcode BAMs and count files rules
 * split_per_bc and featureCount leave behind, CNACalling.smk:17,34, have no counterpart to clean up). */
int lsg_gene_counts_reset(lsg_ctx* ctx);

/* ---- measurement helpers --------------------------------------------------------------------*/
/* Statistics of the last lsg_pileup_count: admitted reads / segments / events (events that passed
 * read admission, before the base-quality gate), tile entries, non-empty units, deep units. */
typedef struct {
    int64_t n_reads_admitted, n_segs_admitted, n_events_admitted;
    int64_t n_entries, n_units, n_deep_units;
    int64_t n_events_wave, n_events_deep;  /* events read by nobody (0) / by the count's range kernel */
    int64_t n_rows_wave, n_rows_deep;      /* rows emitted by each kernel (all cell types)         */
    float   ms_bin, ms_deep, ms_wave, ms_total;   /* HIP-event times of the last call             */
    float   ms_walk;                       /* the range kernel alone (HIP events around the launch) */
    float   pad_;
    int64_t rows_by_kernel[4];             /* rows emitted by: 0 nobody, 1 the count's range kernel (k_tm_walk, k_tm_gather_count, k_tm_count_direct or k_tm_count_win: tiles that are one job), 2 nobody (always 0: a job of the wide walk belongs to a multi-job tile, its sums go to a slab), 3 k_finalize_multi */
    int64_t events_by_kernel[4];           /* events loaded by the same kernels (3 = 0)            */
} lsg_count_stats;
int lsg_get_count_stats(lsg_ctx* ctx, lsg_count_stats* out);

/* What the load's tile store cost.  path: 2 = the store was built by the load alone, 3 = in the pass that also made the first count
 * (lsg_set_count_at_load), 4 = the load made its count and kept no store (lsg_set_store_policy), 5 = the same over tile-phased events
 * (LSG_LAYOUT_PHASED: every entry fetched as its one 128-byte line), 6 = the same with the entries binned by 128-position windows
 * (events phased modulo 128, keys alone through the sort: every entry fetched as one 256-byte block).  build_ms: wall time
 * lsg_load_reads spent building the store (device kernels + their host synchronisations).  store_bytes: device memory the store, its
 * per-read / per-segment arrays, kept events and cached build temporaries hold.  No reference counterpart: the reference re-reads
 * the BAM per window (BaseCellCounter.py:198-225). */
int lsg_get_layout_info(lsg_ctx* ctx, int32_t* path, double* build_ms, int64_t* store_bytes);
/* HIP-event times (ms) of the last load's build phases: [0] capacities + scatter, [1] sort of every tile's entries by barcode,
 * [2] per-entry words, [3] event gather into the transposed blocks (the build's dominant kernel, k_tm_gather). */
int lsg_get_build_times(lsg_ctx* ctx, float* ms4);
/* Shape of the resident tile store: entries ((segment x tile) overlaps of reads with a barcode), 1 KB blocks, and the events the
 * entries hold (what k_tm_gather reads once from the caller's array and writes once: its algorithmic bytes are 4 per event). */
int lsg_get_store_shape(lsg_ctx* ctx, int64_t* n_entries, int64_t* n_blocks, int64_t* n_events);

/* (The synthetic workload of bench.py and the tests - lsg_synth_*, the read-back of resident arrays - is declared in
 * include/longsom_synth.h: measurement and test support, not part of the boundary a rule's script binds.) */

#ifdef __cplusplus
}
#endif
#endif /* LONGSOM_HIP_H */
