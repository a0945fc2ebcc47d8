### MI355X replacement of the counting/calling half of LongSom's workflow/rules/PoN.smk (same OUTPUT files).
#
# The reference maps every normal (minimap2 / samtools / AddBarcodeTag: unchanged, keep those rules), then runs SplitBam ->
# BaseCellCounter -> MergeCounts -> BaseCellCalling.step1 per normal and aggregates the step-1 tables with PoN.py (awk | sort |
# datamash).  Option A (fused): rule PoN_gpu does all of that for all normals in one process per GPU; the per-normal tables are
# written only when config['PoN'].get('tables', True).  Option B: keep the reference's per-normal rules with the drop-in
# scripts of scripts_gpu/SNVCalling (see SNVCalling.gpu.smk) and take only rule PoN_files_gpu, the datamash-free PoN.py.
# BetaBinEstimation.py (VGAM through rpy2) has two replacements, chosen with config['PoN']['fit_on_gpu'] (default False: the
# reference's rule and its conda environment stay in charge of BetaBinEstimates.txt):
#   rule BetaBinEstimation_gpu  the drop-in for BetaBinEstimation_PoN: same input list, same output file, no R;
#   rule PoN_fit_gpu            the fused run with --fit: from normals.tsv to BetaBinEstimates.txt AND PoN_LR.tsv in one process.
# They give the maximum-likelihood estimate (not VGAM's last iterate), over every eligible site by default (PoN.fit_n_sites, 0),
# thinned - when asked to - by a random stream of their own.  The `ruleorder:` below has not been executed: snakemake is not
# installed where this file is tested (tests/test_rules_cpu.py parses the rules' shell lines against the scripts' parsers).

GPU_SCRIPTS = str(workflow.basedir) + "/scripts_gpu"

rule NormalsTable_gpu:
    input:
        bam=expand(f"{DATA}/bam/{{norm}}.bam", norm=NORMS),
        barcodes=expand(f"{DATA}/ctypes/{{norm}}.txt", norm=NORMS),
    output:
        temp(f"{OUTDIR}/PoN/normals.tsv")
    run:
        with open(output[0], "w") as out:
            for n, b, c in zip(NORMS, input.bam, input.barcodes):
                out.write("%s\t%s\t%s\n" % (n, b, c))

rule PoN_gpu:
    input:
        normals=f"{OUTDIR}/PoN/normals.tsv",
        bb=f"{OUTDIR}/PoN/PoN/BetaBinEstimates.txt",
    output:
        f"{OUTDIR}/PoN/PoN/PoN_LR.tsv"
    params:
        script=GPU_SCRIPTS+"/PoN/longsom_gpu_pon.py",
        hg38=config['Global']['genome'],
        mapq=config['SComatic']['BaseCellCounter']['min_mapping_quality'],
        alpha1=lambda w, input: get_BetaBinEstimates(input.bb, 'alpha1'),
        beta1=lambda w, input: get_BetaBinEstimates(input.bb, 'beta1'),
        alpha2=lambda w, input: get_BetaBinEstimates(input.bb, 'alpha2'),
        beta2=lambda w, input: get_BetaBinEstimates(input.bb, 'beta2'),
        p=config['PoN'],
        tables="" if config['PoN'].get('tables', True) else "--no_tables",
        # GPUs of this node used by the rule: the normals are spread over one rank per GPU
        launcher=lambda wc, resources: "python" if resources.gpu == 1 else f"python -m torch.distributed.run --standalone --local-addr 127.0.0.1 --nnodes=1 --nproc-per-node {resources.gpu}",
    resources:
        gpu=config.get('Run', {}).get('gpus', 1)
    shell:
        "{params.launcher} {params.script} --normals {input.normals} --ref {params.hg38} --outdir {OUTDIR} --min_mq {params.mapq} "
        "--alpha1 {params.alpha1} --beta1 {params.beta1} --alpha2 {params.alpha2} --beta2 {params.beta2} "
        "--min_ac_cells {params.p[min_ac_cells]} --min_ac_reads {params.p[min_ac_reads]} --min_cells {params.p[min_cells]} "
        "--min_cell_types {params.p[min_cell_types]} --min_samples 1 --rm_prefix No {params.tables}"

rule PoN_files_gpu:
    input:
        f"{OUTDIR}/PoN/BaseCellCalling/BaseCellCalling_files.txt"
    output:
        f"{OUTDIR}/PoN/PoN/PoN_LR.files.tsv"
    params:
        script=GPU_SCRIPTS+"/PoN/PoN.py",
    shell:
        "python {params.script} --in_tsv {input} --out_file {output} --min_samples 1 --rm_prefix No"

rule BetaBinEstimation_gpu:
    input:
        f"{OUTDIR}/PoN/BaseCellCounter/BaseCellCounter_files.txt"
    output:
        f"{OUTDIR}/PoN/PoN/BetaBinEstimates.txt"
    params:
        script=GPU_SCRIPTS+"/PoN/BetaBinEstimation.py",
        n_sites=config['PoN'].get('fit_n_sites', 0),
        seed=config['PoN'].get('fit_seed', 1992),
    resources:
        gpu=1
    shell:
        "python {params.script} --in_tsv {input} --outfile {output} --n_sites {params.n_sites} --seed {params.seed}"

rule PoN_fit_gpu:
    input:
        normals=f"{OUTDIR}/PoN/normals.tsv",
    output:
        bb=f"{OUTDIR}/PoN/PoN/BetaBinEstimates.txt",
        pon=f"{OUTDIR}/PoN/PoN/PoN_LR.tsv",
    params:
        script=GPU_SCRIPTS+"/PoN/longsom_gpu_pon.py",
        hg38=config['Global']['genome'],
        mapq=config['SComatic']['BaseCellCounter']['min_mapping_quality'],
        p=config['PoN'],
        n_sites=config['PoN'].get('fit_n_sites', 0),
        seed=config['PoN'].get('fit_seed', 1992),
        tables="" if config['PoN'].get('tables', True) else "--no_tables",
        launcher=lambda wc, resources: "python" if resources.gpu == 1 else f"python -m torch.distributed.run --standalone --local-addr 127.0.0.1 --nnodes=1 --nproc-per-node {resources.gpu}",
    resources:
        gpu=config.get('Run', {}).get('gpus', 1)
    shell:
        "{params.launcher} {params.script} --normals {input.normals} --ref {params.hg38} --outdir {OUTDIR} --min_mq {params.mapq} "
        "--fit --fit_n_sites {params.n_sites} --fit_seed {params.seed} "
        "--min_ac_cells {params.p[min_ac_cells]} --min_ac_reads {params.p[min_ac_reads]} --min_cells {params.p[min_cells]} "
        "--min_cell_types {params.p[min_cell_types]} --min_samples 1 --rm_prefix No {params.tables}"

if config['PoN'].get('fit_on_gpu', False):
    if config['PoN'].get('fit_fused', True):
        ruleorder: PoN_fit_gpu > BetaBinEstimation_gpu > BetaBinEstimation_PoN
        ruleorder: PoN_fit_gpu > PoN_gpu
    else:
        ruleorder: BetaBinEstimation_gpu > PoN_fit_gpu > BetaBinEstimation_PoN
        ruleorder: PoN_gpu > PoN_fit_gpu
else:
    ruleorder: BetaBinEstimation_PoN > BetaBinEstimation_gpu > PoN_fit_gpu
    ruleorder: PoN_gpu > PoN_fit_gpu

# The drop-in for IndexBarcodedBam_PoN (PoN.smk:78-96: samtools index of a normal's tagged BAM): the whole .bai - bins, chunks, linear
# index - made on the GPU (longsom_amd.cli index_bam; DESIGN.md section 16 has the file's form).  Optional key PoN.index_device: the GPU.
# It makes the file the reference's rule makes, which stays beside it (the mapping rules of PoN.smk are kept): the `ruleorder:` behind the
# rule leaves IndexBarcodedBam_PoN in charge unless the optional key PoN.index_on_gpu is true.  Like the one above it has not been
# executed: snakemake is not installed where this file is tested.
rule IndexBam_gpu:
    input:
        taggedbam=f"{DATA}/bam/{{norm}}.bam",
    output:
        bai_bc=f"{DATA}/bam/{{norm}}.bam.bai"
    wildcard_constraints:
        norm="([a-zA-Z]+)_Norm"
    params:
        script=GPU_SCRIPTS+"/PreProcessing/IndexBam.py",
        device=(config.get('PoN') or {}).get('index_device', 0),
    shell:
        "python {params.script} --bam {input.taggedbam} --out {output.bai_bc} --device {params.device}"

if config['PoN'].get('index_on_gpu', False):
    ruleorder: IndexBam_gpu > IndexBarcodedBam_PoN
else:
    ruleorder: IndexBarcodedBam_PoN > IndexBam_gpu
