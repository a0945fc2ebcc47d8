/* longsom_synth.h - measurement and test support of liblongsom_hip.so: the synthetic long-read workload of BASELINE.md section 4 generated
 * straight into HBM (bench.py's inputs never cross PCIe), and the read-back of a handle's resident arrays for the CPU oracle.  NOT part of
 * the drop-in boundary (include/longsom_hip.h): nothing a rule's script binds is declared here, and the reference has no counterpart. */
#ifndef LONGSOM_SYNTH_H
#define LONGSOM_SYNTH_H
#include "longsom_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic workload (bench / tests; not part of the reference's path) --------------------*/
/* Gene/expression tables of the BASELINE.md §4 workload model (built by longsom_amd/synth.py; the
 * per-read / per-base draws are counter-based hashes, see longsom_amd/csrc/synth_model.h).
 * All pointers are HOST pointers; celltype_of is ignored on the device path (lsg_set_barcodes's
 * table is used). */
typedef struct {
    uint64_t seed;
    int64_t  n_reads;        /* reads of this (shard of the) model                                 */
    int64_t  read_base;      /* global index of local read 0: draws are keyed by read_base + i, so a
                                shard generates exactly the reads the unsharded model would          */
    int32_t  n_genes, n_cb, n_contigs, snp_mod;
    const int32_t* gene_tid;        /* [G]                                   */
    const int32_t* gene_exon_off;   /* [G+1] index into the exon arrays      */
    const int32_t* exon_start;      /* 0-based reference start of each exon  */
    const int32_t* exon_len;
    const int32_t* exon_cum;        /* transcript coordinate of the exon's first base */
    const int64_t* gene_read_off;   /* [G+1] reads [off[g], off[g+1]) belong to gene g */
    const uint8_t* celltype_of;     /* [n_cb] 0 = Cancer                     */
    int32_t  layout;                /* where the generated events lie: LSG_LAYOUT_COMPACT or LSG_LAYOUT_PHASED (lsg_reads above) */
    int32_t  pad_;
} lsg_synth_model;

/* Fills the reference of every contig with the model's synthetic genome, in HBM. */
int lsg_synth_reference(lsg_ctx* ctx, uint64_t seed);
/* Generates the model's read-record arrays directly in HBM and makes them the loaded reads (generate + lsg_load_reads). */
int lsg_synth_reads(lsg_ctx* ctx, const lsg_synth_model* model);
/* Only generates them: *out describes compact device arrays owned by the handle (valid until the next generate, lsg_synth_reads or
 * lsg_destroy) — a stand-in for a caller whose decoded BAM is device-resident; bench.py times lsg_load_reads on them. */
int lsg_synth_generate(lsg_ctx* ctx, const lsg_synth_model* model, lsg_reads* out);
int lsg_get_reads_shape(lsg_ctx* ctx, int64_t* n_reads, int64_t* n_segs, int64_t* n_events);
/* Copies the resident read-record arrays / reference into caller-allocated host arrays.  out->events and out->seg_ev_off both NULL:
 * the per-read and per-segment arrays only (always resident: what a sharded run cuts its regions from); otherwise the events too, which
 * are there only when the load kept them (lsg_set_keep_reads). */
int lsg_copy_reads_to_host(lsg_ctx* ctx, const lsg_reads* out);
int lsg_copy_reference_to_host(lsg_ctx* ctx, int32_t tid, uint8_t* out);

/* ---- the BnpC sampler's parts, one at a time (csrc/bnpc_sampler.hip; tests/test_bnpc_sampler_gpu.py) ---------------------------------
 * lsg_bnpcs_test_stream: the Philox words [n][4] and the two doubles [n][2] of counters [n][4] under a key, as the kernels form them.
 * lsg_bnpcs_test_variates: n variates with index i = 0 .. n-1 at step 0: kind 0 Beta(a, b) under purpose P_BIRTH, kind 1 the truncated
 *   normal around a (float32) with sd b at the first double of purpose P_MH, kind 2 Gamma(a) under P_ALPHA; *errors: tries run out.
 * The others work on the state lsg_bnpcs_set_state loaded: _test_counts copies out n1, n0 [n_cells][n_muts] of a chain; _test_ll makes the
 * likelihood matrix and copies out ll [n_cells][*n_clusters] and the cluster ids of its columns; _test_move makes one sweep with its
 * concentration update (what = 0), one parameter move (what = 1), one split-merge move with its concentration update (what = 2: every
 * chain takes it, whatever its deciding draw says) or one error-rate update (what = 3: a chain makes it where its deciding draw says so
 * under lsg_bnpcs_set_error_learning's probability) of every chain under the step number `step`, recording nothing.
 * lsg_bnpcs_test_move_outcome: a chain's last split-merge move, outcome [12]: the code as in lsg_bnpcs_fetch_moves, the two cluster ids (a
 * split: the cluster and the smallest free id), the two anchors, A, its four terms in the order they are added, ln v, |S|.
 * lsg_bnpcs_test_error_outcome: a chain's last error-rate update (what = 3), outcome [21]: 1 if the deciding draw said update, else 0; then
 * for FP and for FN ten numbers: the index of the proposal's sd, the proposed rate, new_ll, old_ll, new_prior - old_prior, new_p_target,
 * old_p_target, A, ln v, the decision (1 accepted, 0 declined, -1 declined because rounding put the proposal at <= 0 or >= 1).
 * lsg_bnpcs_test_set_ml: writes values [n] as the ML records first .. first + n - 1 of a chain, so that lsg_bnpcs_psrf can be held to given
 * series; lsg_bnpcs_psrf then takes the records below first + n as made.  Refused: records past the room lsg_bnpcs_create / _extend made. */
int lsg_bnpcs_test_stream(lsg_ctx* ctx, uint64_t key, int64_t n, const uint32_t* counters, uint32_t* words, double* doubles);
int lsg_bnpcs_test_variates(lsg_ctx* ctx, uint64_t key, int32_t kind, int64_t n, double a, double b, double* out, int32_t* errors);
int lsg_bnpcs_test_counts(lsg_ctx* ctx, int32_t chain, uint32_t* n1, uint32_t* n0);
int lsg_bnpcs_test_ll(lsg_ctx* ctx, int32_t chain, double* ll, int32_t* clusters, int32_t* n_clusters);
int lsg_bnpcs_test_move(lsg_ctx* ctx, int32_t what, int32_t step);
int lsg_bnpcs_test_move_outcome(lsg_ctx* ctx, int32_t chain, double* outcome);
int lsg_bnpcs_test_error_outcome(lsg_ctx* ctx, int32_t chain, double* outcome);
int lsg_bnpcs_test_set_ml(lsg_ctx* ctx, int32_t chain, int32_t first, int32_t n, const double* values);

#ifdef __cplusplus
}
#endif
#endif /* LONGSOM_SYNTH_H */
