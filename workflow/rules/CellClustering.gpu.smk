### MI355X replacement of rule SingleCellGenotype of LongSom's workflow/rules/CellClustering.smk (same INPUT and OUTPUT files, same flags).
#
# The reference states the rule twice (PoN run or not): the two differ only in where alpha2 / beta2 come from - the panel's
# BetaBinEstimates.txt or config['SNVCalling']['BaseCellCalling'] - and that is the one conditional here.  FormatInputBnpC and
# BnpC_clustering read the matrices this rule writes and stay the reference's.

GPU_SCRIPTS = str(workflow.basedir) + "/scripts_gpu"

rule SingleCellGenotype:
    input:
        tsv="SNVCalling/BaseCellCalling/{id}.calling.step3.tsv",
        bam=f"{INPUT}/bam/{{id}}.bam",
        barcodes="CellTypeReannotation/ReannotatedCellTypes/{id}.tsv",
        bb="PoN/PoN/BetaBinEstimates.txt" if PON else [],
        fusions="FusionCalling/Somatic/{id}.Fusions.SingleCellGenotype.tsv" if CTATFUSION else [],
        ref=str(workflow.basedir)+config['Reference']['genome'],
    output:
        tsv="CellClustering/SingleCellGenotype/{id}.SingleCellGenotype.tsv",
        dp="CellClustering/SingleCellGenotype/{id}.DpMatrix.tsv",
        alt="CellClustering/SingleCellGenotype/{id}.AltMatrix.tsv",
        vaf="CellClustering/SingleCellGenotype/{id}.VAFMatrix.tsv",
        bin="CellClustering/SingleCellGenotype/{id}.BinaryMatrix.tsv",
        tmp=temp(directory("CellClustering/SingleCellGenotype/{id}/"))
    params:
        script=GPU_SCRIPTS+"/CellClustering/SingleCellGenotype.py",
        alt_flag=config['CellClust']['SingleCellGenotype']['alt_flag'],
        mapq=config['SNVCalling']['BaseCellCounter']['min_mapping_quality'],
        alpha2=lambda w, input: get_BetaBinEstimates(input.bb, 'alpha2') if PON else config['SNVCalling']['BaseCellCalling']['alpha2'],
        beta2=lambda w, input: get_BetaBinEstimates(input.bb, 'beta2') if PON else config['SNVCalling']['BaseCellCalling']['beta2'],
        pval=config['CellClust']['SingleCellGenotype']['pvalue'],
        chrm_conta=config['SNVCalling']['BaseCellCalling']['chrM_contaminant'],
        # Run.htslib_legacy_del_merge: True counts CIGAR 1D2D's first deleted column as 'D' (pysam over htslib <= 1.10); default: htslib >= 1.11
        htslib="--htslib_legacy_del_merge" if config['Run'].get('htslib_legacy_del_merge', False) else "",
    resources:
        gpu=1
    log:
        "logs/SingleCellGenotype/{id}.log",
    benchmark:
        "benchmarks/SingleCellGenotype/{id}.benchmark.txt"
    shell:
        r"""
        python {params.script} \
        --infile {input.tsv} \
        --outfile CellClustering/SingleCellGenotype/{wildcards.id} \
        --bam {input.bam} \
        --meta {input.barcodes} \
        --ref {input.ref} \
        --fusions {input.fusions} \
        --nprocs {threads} \
        --min_mq {params.mapq} \
        --pvalue {params.pval} \
        --alpha2 {params.alpha2} \
        --beta2 {params.beta2} \
        --alt_flag {params.alt_flag} \
        --chrM_contaminant {params.chrm_conta} \
        --tmp_dir {output.tmp} {params.htslib}
        """
