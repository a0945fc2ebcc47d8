### MI355X replacement of LongSom's workflow/rules/FusionCalling.smk (same OUTPUT files).
#
# Option A (fused): rule FusionFastq_gpu prints FusionCalling/{id}/{id}.fastq straight from the unsplit BAM and the barcode table that
# SplitBam_gpu takes: the records SplitBamCellTypes would write per cell type, cell type after cell type.  It replaces the per-cell-type
# BAMs, the two BamToFastq runs and ConcatFastq (FusionCalling.smk:3-37); the text is printed on the device and streamed into the file
# with lsg_append_table, as the fused SNV rule streams its tables.
# Option B (drop-in): keep SplitBam_gpu and ConcatFastq and take rule BamToFastq below, the reference's rule over scripts_gpu.
# Rule CTATFusion (ctat-LR-fusion in its container) is not touched: keep it from FusionCalling.smk.  Rule SomaticFusions is the
# reference's with the drop-in script.  `include: "rules/FusionCalling.gpu.smk"` beside the rules kept from FusionCalling.smk.

GPU_SCRIPTS = str(workflow.basedir) + "/scripts_gpu"

# SplitBamCellTypes' --max_nM / --max_NH from the optional config['SNVCalling']['SplitBam'], as in SNVCalling.gpu.smk (n_trim is not
# supported here: a trimmed read's FASTQ qualities would differ)
FUSION_SPLIT_FILTERS = {k: ("" if v is None else v) for k, v in
                        {"max_nM": None, "max_NH": None, **{k: v for k, v in (config['SNVCalling'].get('SplitBam') or {}).items() if k != "n_trim"}}.items()}

rule FusionFastq_gpu:
    input:
        bam=f"{INPUT}/bam/{{id}}.bam",
        barcodes="CellTypeReannotation/ReannotatedCellTypes/{id}.tsv" if REANNO else "Barcodes/{id}.tsv",
    output:
        fastq=temp("FusionCalling/{id}/{id}.fastq")
    params:
        script=GPU_SCRIPTS+"/FusionCalling/longsom_gpu_fastq.py",
        mapq=config['SNVCalling']['BaseCellCounter']['min_mapping_quality'],
        max_nm=FUSION_SPLIT_FILTERS['max_nM'], max_nh=FUSION_SPLIT_FILTERS['max_NH'],
    log:
        "logs/FusionFastq/{id}.log",
    benchmark:
        "benchmarks/FusionFastq/{id}.benchmark.txt"
    shell:
        "python {params.script} --bam {input.bam} --meta {input.barcodes} --id {wildcards.id} --outdir FusionCalling/{wildcards.id} --min_MQ {params.mapq} "
        "--max_nM={params.max_nm} --max_NH={params.max_nh}"

rule BamToFastq:
    input:
        bam="SNVCalling/SplitBam/{id}.{celltype}.bam"
    output:
        fastq=temp("FusionCalling/{id}/{id}.{celltype}.fastq")
    params:
        script=GPU_SCRIPTS+"/FusionCalling/BamToFastq.py",
    log:
        "logs/BamToFastq/{id}.{celltype}.log",
    benchmark:
        "benchmarks/BamToFastq/{id}.{celltype}.benchmark.txt"
    shell:
        "python {params.script} --bam {input.bam} --fastq {output.fastq}"

rule SomaticFusions:
    input:
        fusions="FusionCalling/{id}/ctat-LR-fusion.fusion_predictions.tsv",
        barcodes="CellTypeReannotation/ReannotatedCellTypes/{id}.tsv" if REANNO else "Barcodes/{id}.tsv"
    output:
        fusions="FusionCalling/Somatic/{id}.Fusions.tsv",
        long="FusionCalling/Somatic/{id}.Fusions.SingleCellGenotype.tsv"
    params:
        script=GPU_SCRIPTS+"/FusionCalling/FusionCalling.py",
        deltaMCF=config['FusionCalling']['SomaticFusions']['deltaMCF'],
        min_ac_reads=config['FusionCalling']['SomaticFusions']['min_ac_reads'],
        min_ac_cells=config['FusionCalling']['SomaticFusions']['min_ac_cells'],
        max_MCF_noncancer=config['FusionCalling']['SomaticFusions']['max_MCF_noncancer'],
    log:
        "logs/SomaticFusions/{id}.log",
    benchmark:
        "benchmarks/SomaticFusions/{id}.benchmark.txt"
    shell:
        "python {params.script} --fusions {input.fusions} --barcodes {input.barcodes} --min_ac_reads {params.min_ac_reads} "
        "--min_ac_cells {params.min_ac_cells} --max_MCF_noncancer {params.max_MCF_noncancer} --deltaMCF {params.deltaMCF} "
        "--outdir FusionCalling/Somatic/{wildcards.id}"
