"""Where longsom_amd/csrc/*.hip sizes a grid from the device's CU count (lsg_ctx::n_cus), and which test takes that launch past the
cap: the host caps the grid and the kernel walks the rest (`for (i = first; i < n; i += stride)`, or a queue the workers pull from),
so an input below the cap gives every worker at most one trip and never runs the loop's step, the scratch a worker clears between
trips, or the barrier between one trip's last read and the next one's first write.

LAUNCHES holds one entry per such place.  `match` is the source line's own text around n_cus (tests/test_grid_caps_cpu.py finds the
line by it, so line numbers may move); `cap(cu)` the work items one trip of the whole grid takes at `cu` CUs; `unit` what one worker
takes per trip.  Then EITHER `test`, the GPU test sized from cu_count() that takes the kernel past twice its cap, OR `why`, one sentence
on why no small input can, with `covered_by`, the at-scale tests whose sizes (read from those tests and stated in `why`) do.
OTHER_USES lists the lines that read n_cus and size no grid."""
from collections import namedtuple

import torch        # at import, before any Engine loads the HIP library: two copies of the HIP runtime in one process, the library's loaded
                    # first, leave torch without a device ("No HIP GPUs are available"); loaded after torch's, the library shares it

Launch = namedtuple("Launch", "file kernel match cap unit test why covered_by", defaults=(None, None, ()))
Other = namedtuple("Other", "file match what")


def cu_count() -> int:
    """the device's CU count, the number lsg_create stores in n_cus (256 on a whole MI355X, fewer on a partition)"""
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def past(cap: int, extra: int) -> int:
    """2 * cap + extra items with 0 < extra < cap: `extra` workers make three trips, the rest two"""
    assert 0 < extra < cap, (cap, extra)
    return 2 * cap + extra


def trips(n: int, cap: int) -> int:
    """the trips the busiest worker makes over n items"""
    return -(-n // cap)


CAPS = "tests/test_grid_caps_gpu.py::"
FULL = "tests/test_fullsize_gpu.py::test_full_size_rows_equal_the_cpu_oracle"
INGEST = "tests/test_ingest_gpu.py::test_the_whole_device_ingest_path_at_scale"
QUEUE = "tests/test_bgzf_shapes_gpu.py::test_queue"
WARD = "tests/test_bnpc_linkage_gpu.py::test_tree_cuts_and_count_against_scipy"
CALLS = "tests/test_call_gpu.py::test_step1_matches_reference_golden"

LAUNCHES = [
    # ---- the peripheral kernels: each has a test of its own, sized from the CU count ----------------------------------------------
    Launch("fastq.hip", "k_fq_print", "unsigned g = (unsigned)((n_rec + 3) / 4); const unsigned cap = (unsigned)(c->n_cus * 32);",
           lambda cu: 32 * cu * 4, "a wave per record", test=CAPS + "test_fastq_print_past_the_cap"),
    Launch("bnpc.hip", "k_bnpc_pack", "(total + 255) / 256, (int64_t)c->n_cus * 32)",
           lambda cu: 32 * cu * 256, "a thread per padded label", test=CAPS + "test_bnpc_estimate_past_the_caps"),
    Launch("bnpc.hip", "k_bnpc_criteria", "std::min<int64_t>(b.n_samples, (int64_t)c->n_cus * 4)",
           lambda cu: 4 * cu, "a workgroup per sample", test=CAPS + "test_bnpc_estimate_past_the_caps"),
    Launch("bnpc_linkage.hip", "k_bnpc_cluster_counts", "std::min<int64_t>(b.n_samples, (int64_t)c->n_cus * 8)",
           lambda cu: 8 * cu, "a workgroup per sample", test=CAPS + "test_bnpc_estimate_past_the_caps"),
    Launch("cellgeno.hip", "k_cell_classify", "unsigned blocks = (unsigned)((cells + 255) / 256); if (blocks > (unsigned)(c->n_cus * 32))",
           lambda cu: 32 * cu * 256, "a thread per cell", test=CAPS + "test_cell_verdicts_past_the_cap"),
    Launch("cellgeno.hip", "k_cells_status", "unsigned blocks = (unsigned)((cells + 255) / 256); if (blocks > (unsigned)(c->n_cus * 32))",
           lambda cu: 32 * cu * 256, "a thread per cell", test=CAPS + "test_loaded_cells_past_the_cap"),
    Launch("call.hip", "k_sf4_batch", "unsigned g = (unsigned)((items + 255) / 256); if (g > (unsigned)(c->n_cus * 16))",
           lambda cu: 16 * cu * 256, "a thread per (k, n) pair", test=CAPS + "test_betabinom_sf4_past_the_cap"),
    Launch("bbfit.hip", "k_bbfit_accumulate", "want = (c->n_ne + 3) / 4, most = (uint32_t)c->n_cus * 4u",
           lambda cu: 4 * cu * 4, "a wave per 64-position unit", test=CAPS + "test_bbfit_accumulate_past_the_cap"),
    # ---- launches only a large input takes past the cap: the at-scale tests stand for them ------------------------------------------
    Launch("bnpc_linkage.hip", "k_bnpc_ward_fill", "((int64_t)n * n + 255) / 256, (int64_t)c->n_cus * 32)",
           lambda cu: 32 * cu * 256, "a thread per element of the N x N working matrix",
           why="the matrix has N x N elements and the tree behind it is compared with scipy's, which takes seconds past N = 2049: that shape's "
               "4 198 401 elements are just over twice the cap of a whole device.", covered_by=(WARD,)),
    Launch("ingest.hip", "k_inflate", "unsigned g = (n_blk + 63) / 64; const unsigned cap = (unsigned)c->n_cus * (per_cu ? per_cu : 5u);",
           lambda cu: 5 * cu * 64, "a lane per BGZF member, the rest off a queue",
           why="a member per lane needs a file of more members than the grid has lanes, which test_queue writes from the CU count "
               "(64 x 5 x CUs + 1 502 members); it is the file-sized test of this launch already.", covered_by=(QUEUE,)),
    Launch("ingest.hip", "k_block_crc", "unsigned g = (n_blk + 3) / 4; const unsigned cap = (unsigned)(c->n_cus * 8);",
           lambda cu: 8 * cu * 4, "a wave per BGZF member",
           why="the same files: test_queue's 64 x 5 x CUs + 1 502 members are ten times the cap, the 24 k members of the 1.5 M-read BAM three times.",
           covered_by=(QUEUE, INGEST)),
    Launch("ingest.hip", "k_rec_emit", "unsigned g = (unsigned)((n_rec + 3) / 4); const unsigned cap = (unsigned)(c->n_cus * 32);",
           lambda cu: 32 * cu * 4, "a wave per record",
           why="a record per wave needs a BAM of more records than 128 x CUs: test_queue's has 64 x 5 x CUs + 1 500 (2.5 times the cap), the "
               "at-scale load 1.5 M.", covered_by=(QUEUE, INGEST)),
    Launch("call.hip", "k_tail_table", "hipLaunchKernelGGL(k_tail_table, dim3((unsigned)(c->n_cus * 8))",
           lambda cu: 8 * cu * 256, "a thread per entry of the small-n tail table",
           why="the table's size is fixed (2 x 2048 x 2049 / 2 = 4.2 M entries, eight times the cap of a whole device), so every first call "
               "of a parameter set walks it in several trips and every compared call reads it.", covered_by=(CALLS, FULL)),
    Launch("call.hip", "k_call_gather", "const unsigned gather_grid = (unsigned)(c->n_cus * 4);",
           lambda cu: 4 * cu * 4, "a wave per chunk of tile heads",
           why="a fixed grid over the tiles that hold sites: it takes the 23.9 M merged sites of the full C2 workload to give every wave many "
               "chunks, and its output is pinned there by the oracle's digest of the candidate rows.", covered_by=(FULL,)),
    Launch("call.hip", "k_call_tails", "hipLaunchKernelGGL(k_call_tails, dim3((unsigned)(c->n_cus * 16))",
           lambda cu: 16 * cu * 256, "a thread per light tail task",
           why="tail tasks come from merged sites the table does not answer (0.08 a site on C2): only the full workload's 23.9 M sites make "
               "more than 16 x CUs x 256 of them.", covered_by=(FULL,)),
    Launch("call.hip", "k_call_tails_heavy", "hipLaunchKernelGGL(k_call_tails_heavy, dim3((unsigned)(c->n_cus * 8))",
           lambda cu: 8 * cu * 4 * 16, "a wave per batch of 16 heavy task slots, off a queue",
           why="heavy tasks are rarer still than light ones and come only from deep sites: the full workload's call is the one test with sites deep enough "
               "to queue them in number; how many is pinned nowhere, so a wave may still take a single batch there.",
           covered_by=(FULL,)),
    Launch("call.hip", "k_call_finish", "hipLaunchKernelGGL(k_call_finish, dim3((unsigned)(c->n_cus * 2))",
           lambda cu: 2 * cu * 256, "a thread per deferred site",
           why="deferred sites are a small share of the merged ones: the full C2 workload lists 294 k of its 23.9 M, twice the cap of a whole device.",
           covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_walk", 'L.grid_walk = (unsigned)(c->n_cus * tune_int("LSG_GRID_TM", 16));',
           lambda cu: 16 * cu, "a workgroup per job of the tile store",
           why="jobs are tiles' worth of entries: it takes millions of reads to make more than 16 x CUs of them, and the store-keeping load "
               "of the full workloads (10 M and 50 M reads, 47.5 M and 48.0 M rows) does.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_finalize_multi", "L.grid_fin = (unsigned)(c->n_cus * 8);",
           lambda cu: 8 * cu, "a workgroup per multi-job tile",
           why="multi-job tiles are the deep ones: the full C2 workload has 6 600 of them among its 500 k non-empty tiles (DESIGN.md section 3), "
               "three times the cap of a whole device; nothing smaller comes near.",
           covered_by=(FULL,)),
    Launch("pileup.hip", "k_prep_ops", "hipLaunchKernelGGL(k_prep_ops, dim3((unsigned)(c->n_cus * 4))",
           lambda cu: 4 * cu * 256, "a thread per 16 bytes of the count's buffers to clear or copy",
           why="the buffers grow with the tiles of the load; the full workloads' are gigabytes, thousands of trips a thread.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_read_stats", "unsigned g = (unsigned)((R + 255) / 256); if (g > (unsigned)(c->n_cus * 8))",
           lambda cu: 8 * cu * 256, "a thread per read",
           why="a read per thread: 10 M and 50 M reads against a cap of 8 x CUs x 256.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_walk_wide", "const unsigned grid_wide = c->tm_n_wide ?",
           lambda cu: 4 * cu, "a wave per wide job",
           why="wide jobs hold 4 096 entries or more in one tile, which only the full workloads' depth (C4: tiles of more than 200 000 reads) "
               "makes in number; how many is pinned nowhere, so this launch may still run below its cap there.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_count_win", 'const unsigned gridw = (unsigned)(c->n_cus * tune_int("LSG_GRID_TW", 9));',
           lambda cu: 9 * cu, "a workgroup per window job",
           why="the one-shot count by windows of the full workloads (their first form: path 6) queues far more window jobs than 9 x CUs.",
           covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_count_direct", 'const unsigned grid = (unsigned)(c->n_cus * tune_int("LSG_GRID_TD", 12));',
           lambda cu: 12 * cu, "a workgroup per tile job",
           why="the one-shot count by tiles of the full workloads (their second form: path 4) queues far more tile jobs than 12 x CUs.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_gather_count", 'const unsigned grid = (unsigned)(c->n_cus * tune_int("LSG_GRID_TG", 9));',
           lambda cu: 9 * cu, "a workgroup per tile job",
           why="the count inside a store-building load; the full workloads' third form builds the store over 10 M and 50 M reads.", covered_by=(FULL,)),
    Launch("pileup.hip", "k_tm_walk_wide", "const dim3 grid_wide((unsigned)(c->n_cus * 2));",
           lambda cu: 2 * cu, "a wave per wide job, their number read on the device",
           why="as the wide walk above, behind the one-shot counts: the same jobs, the same caveat.", covered_by=(FULL,)),
    Launch("store.hip", "k_seg_static", "if (g_seg > (unsigned)(c->n_cus * 16)) g_seg = (unsigned)(c->n_cus * 16);",
           lambda cu: 16 * cu * 256 * 4, "a thread per four segments",
           why="a load's segments: more than 16 x CUs x 1 024 of them need millions of reads (the full workloads' 10 M and 50 M).",
           covered_by=(FULL,)),
    Launch("store.hip", "k_bin", "if (b.g_bin > (unsigned)(c->n_cus * 8)) b.g_bin = (unsigned)(c->n_cus * 8);",
           lambda cu: 8 * cu * 256 * 16, "a workgroup per super-batch of 4 096 segments, off a queue",
           why="the same segments against 8 x CUs x 4 096.", covered_by=(FULL,)),
]

OTHER_USES = [
    Other("lsg_api.hip", "c->n_cus = prop.multiProcessorCount;", "where the count is read"),
    Other("pileup.hip", "const uint64_t emitters = (uint64_t)L.grid_walk * TMW_WAVES * 2", "the row arenas' size, from the grids above"),
    Other("store.hip", "const uint64_t per = N / ((uint64_t)c->n_cus * 14 * 4);", "a job's target length"),
    Other("store.hip", "const uint64_t cw = total_work / ((uint64_t)c->n_cus * 14 * 6);", "a job's target work"),
]
