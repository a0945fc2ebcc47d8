### MI355X replacement of rules SingleCellGenotype, FormatInputBnpC and BnpC_clustering of LongSom's workflow/rules/CellClustering.smk (same
### INPUT and OUTPUT files, same flags).
#
# The reference states SingleCellGenotype twice (PoN run or not): the two differ only in where alpha2 / beta2 come from - the panel's
# BetaBinEstimates.txt or config['SNVCalling']['BaseCellCalling'] - and that is the one conditional here.  FormatInputBnpC filters the
# Binary and VAF matrices into BnpC's input; with Run.fuse_bnpc_input: True rule SingleCellGenotype writes that input in its own process,
# from the cells while they are resident, and FormatInputBnpC has nothing left to do (the rule order below gives the files to the fused
# rule).  BnpC_clustering reads BnpC_input/: its sampler is the vendored BnpC's of this checkout (scripts/CellClustering/libs), run as the
# reference runs it; the posterior estimate over the chains' samples runs on the GPU.  With CellClust.BnpC.sampler: device-sm the sampler
# runs on the GPU too, all chains at once, with the reference's own settings: Gibbs sweeps, the split-merge move in a third of the steps
# (--sampler device-sm, no -smp passed, so run_BnpC.py's defaults -smp 0.33 -sms 3 -smr 0.75 0.25 apply as in the reference's rule), the
# parameter moves, fixed error rates.  CellClust.BnpC.sampler: device is the same without the split-merge move (--sampler device -smp 0).
# CellClust.BnpC.sampler: device-errors is device-sm with the error rates learned (--sampler device-errors): the rule passes the config's
# -eup, and any value of it runs on the GPU, where device and device-sm need eup: 0.  CellClust.BnpC.sampler: device-open is device-errors
# with chains of open length (--sampler device-open): with the optional key CellClust.BnpC.lugsail the rule passes it as -ls, and the chains
# run until their lugsail PSRF is at most that cutoff (which overrides -s, as in run_BnpC.py); without the key it equals device-errors.

GPU_SCRIPTS = str(workflow.basedir) + "/scripts_gpu"
FUSE_BNPC = config['Run'].get('fuse_bnpc_input', False)
BNPC_INPUT = dict(bnpc_bin="CellClustering/BnpC_input/{id}.BinaryMatrix.tsv",
                  bnpc_vaf="CellClustering/BnpC_input/{id}.VAFMatrix.tsv",
                  bnpc_barcodes="CellClustering/BnpC_input/{id}.Barcodes.tsv") if FUSE_BNPC else {}

ruleorder: SingleCellGenotype > FormatInputBnpC

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
        tmp=temp(directory("CellClustering/SingleCellGenotype/{id}/")),
        **BNPC_INPUT
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
        # the fused form: a prefix, or nothing (a bare --bnpc_outfile: no BnpC input is written)
        bnpc_outfile=lambda w: ("CellClustering/BnpC_input/" + w.id) if FUSE_BNPC else "",
        min_cells=config['CellClust']['FormatInput']['min_cells_per_mut'],
        min_cov=config['CellClust']['FormatInput']['min_pos_cov'],
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
        --min_cells_per_mut {params.min_cells} \
        --min_pos_cov {params.min_cov} \
        --bnpc_outfile {params.bnpc_outfile} \
        --tmp_dir {output.tmp} {params.htslib}
        """

rule FormatInputBnpC:
    input:
        bin="CellClustering/SingleCellGenotype/{id}.BinaryMatrix.tsv",
        vaf="CellClustering/SingleCellGenotype/{id}.VAFMatrix.tsv",
        barcodes="CellTypeReannotation/ReannotatedCellTypes/{id}.tsv",
    output:
        bin="CellClustering/BnpC_input/{id}.BinaryMatrix.tsv",
        vaf="CellClustering/BnpC_input/{id}.VAFMatrix.tsv",
        barcodes="CellClustering/BnpC_input/{id}.Barcodes.tsv",
    params:
        script=GPU_SCRIPTS+"/CellClustering/FormatInputBnpC.py",
        min_cells=config['CellClust']['FormatInput']['min_cells_per_mut'],
        min_cov=config['CellClust']['FormatInput']['min_pos_cov'],
    resources:
        gpu=1
    log:
        "logs/FormatInputBnpC/{id}.log",
    benchmark:
        "benchmarks/FormatInputBnpC/{id}.benchmark.txt"
    shell:
        r"""
        python {params.script} \
        --bin {input.bin} \
        --vaf {input.vaf} \
        --barcodes {input.barcodes} \
        --min_pos_cov {params.min_cov} \
        --min_cells_per_mut {params.min_cells} \
        --outfile CellClustering/BnpC_input/{wildcards.id}
        """

rule BnpC_clustering:
    input:
        bin="CellClustering/BnpC_input/{id}.BinaryMatrix.tsv",
        vaf="CellClustering/BnpC_input/{id}.VAFMatrix.tsv",
        barcodes="CellClustering/BnpC_input/{id}.Barcodes.tsv",
    output:
        pdf="CellClustering/BnpC_output/{id}/genoCluster_posterior_mean_raw.pdf"
    params:
        script=GPU_SCRIPTS+"/CellClustering/run_BnpC.py",
        mcmc_steps = config['CellClust']['BnpC']['mcmc_steps'],
        estimator = config['CellClust']['BnpC']['estimator'],
        dpa = config['CellClust']['BnpC']['dpa'],
        cup = config['CellClust']['BnpC']['cup'],
        eup = config['CellClust']['BnpC']['eup'],
        FP = config['CellClust']['BnpC']['FP'],
        FN = config['CellClust']['BnpC']['FN'],
        pp= config['CellClust']['BnpC']['pp'],
        sampler={'device': "--sampler device -smp 0", 'device-sm': "--sampler device-sm", 'device-errors': "--sampler device-errors",
                 'device-open': "--sampler device-open"}.get(config['CellClust']['BnpC'].get('sampler', 'reference'), ""),
        lugsail=("-ls %s" % config['CellClust']['BnpC']['lugsail']) if 'lugsail' in config['CellClust']['BnpC'] else "",
    conda:
        "../envs/BnpC.yaml"
    threads: 16
    resources:
        mem_mb_per_cpu=1024,
        gpu=1
    log:
        "logs/BnpC/{id}.log",
    benchmark:
        "benchmarks/BnpC/{id}.benchmark.txt"
    shell:
        r"""
        python {params.script} \
        {input.bin} \
        -n {threads} \
        -o CellClustering/BnpC_output/{wildcards.id} \
        -s {params.mcmc_steps} \
        -e {params.estimator} \
        -cup {params.cup} \
        -eup {params.eup} \
        -FP {params.FP} \
        -FN {params.FN} \
        -pp {params.pp} \
        -ap {params.dpa} {params.sampler} {params.lugsail} \
        --barcodes {input.barcodes}
        """
