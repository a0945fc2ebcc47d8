### MI355X replacement of the counting half of LongSom's workflow/rules/CNACalling.smk (same OUTPUT file).
#
# Rule GeneCounts_gpu writes InferCNV/featurecount/output/{id}.counts.formated.txt, the cell-by-gene read counts ctat_infercnv reads,
# straight from the unsplit BAM, the barcode table and the annotation.  It replaces rules split_per_bc (one BAM per barcode),
# featureCount (featureCounts -L over all of them) and format_featureCount (names for ids, rows summed by name): CNACalling.smk:11-75.
# A read's barcode is resident after the load, so nothing is split; the reads are assigned to genes and the matrix is printed on the
# device.  What is counted is stated in longsom_amd/genecounts.py and DESIGN.md §13: featureCounts' defaults (-t exon -g gene_id -s 0,
# no -O, -Q 0), without the NH rule of a run without -M (minimap2 writes no NH).
# --tsv: the matrix is tab-separated, which is what infercnv.R:14 reads (the reference's format_featureCount writes commas).
# Rule ctat_infercnv (inferCNV in its conda environment) is not touched: keep it from CNACalling.smk.
# `include: "rules/CNACalling.gpu.smk"` beside the rule kept from CNACalling.smk.

GPU_SCRIPTS = str(workflow.basedir) + "/scripts_gpu"

rule GeneCounts_gpu:
    input:
        bam=f"{INPUT}/bam/{{id}}.bam",
        barcodes="CellTypeReannotation/ReannotatedCellTypes/{id}.tsv" if REANNO else "Barcodes/{id}.tsv",
        gtf=config['Global']['isoforms'],
    output:
        counts="InferCNV/featurecount/output/{id}.counts.formated.txt",
        summary="InferCNV/featurecount/output/{id}.counts.summary.tsv",
    params:
        script=GPU_SCRIPTS+"/CNACalling/longsom_gpu_gene_counts.py",
        gene_names=(config.get('inferCNV') or {}).get('gene_names', 'third'),
    log:
        "logs/GeneCounts/{id}.log",
    benchmark:
        "benchmarks/GeneCounts/{id}.benchmark.txt"
    shell:
        "python {params.script} --bam {input.bam} --meta {input.barcodes} --gtf {input.gtf} --id {wildcards.id} "
        "--outdir InferCNV/featurecount/output --gene_names {params.gene_names} --tsv"
