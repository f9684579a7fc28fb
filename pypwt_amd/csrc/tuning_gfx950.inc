// tuning_gfx950.inc -- the dispatch thresholds of the MI355X (gfx950) build as DATA, one row per rule:
//
//     PDWT_TUNE(key, value, "evidence", "measured", "what the value decides")
//
// `evidence` is the measurement the value comes from (a file under profiles/, or docs/LAB_NOTEBOOK.md for rounds 1-3 whose raw
// files are summarised there); `measured` the round and date.  plan.cpp (build_schedule) and the launch_*.hip dispatchers read
// the values as pdwt::tune::key (tuning.hpp); tools/tuning_table.py prints this file as the table of DESIGN.md and checks that
// every evidence file exists; tools/retune.py re-measures the keys a process can move at run time (pdwt_set_tuning) and says
// which rows a sweep would change.  The run-time keys themselves ("tuning key ..." below) are the rows of tuning_knobs.inc.
//
// Rule for changing a value (VERDICT round 5, weak 6): an A/B may move a default only when the alternative wins by at least
// 5 % on the measured plan, or by any margin on three different boxes -- box-to-box spread on 10-90 us plans is 2-10 %
// (cfg2: 70.4-72.9 us over ten boxes in round 5), which is what most of the margins behind these rows were measured inside of.
//
// All sizes are SAMPLES ENTERING THE LAUNCH (batch x rows x columns of the level's input) as log2, unless said otherwise.

// ---- 2D DWT: which kernel family serves a LEVEL launch (launch_dwt2.hip)
PDWT_TUNE(wave_min_log2,        22, "docs/LAB_NOTEBOOK.md",                   "round 2, 2026-10",  "wave-per-tile kernels (<= 8 taps) from 2^v samples; 63 = never; tuning key wave_min_log2")
PDWT_TUNE(wave_min_log2_f64,    16, "profiles/r04zn_f64scan_after.txt",                   "round 4",           "the same in the fp64 library (no tuned LDS tiles to prefer)")
PDWT_TUNE(lds_max_log2,         25, "profiles/r04za_ab_batchrange.txt",         "round 4",           "LDS tiles preferred to the wave kernels up to 2^v samples; tuning key lds_max_log2")
PDWT_TUNE(lds_tiles_above_log2, 22, "profiles/r02y_kbench_tiles.txt",         "round 2",           "... and only above 2^v (the 2048^2 level of cfg2 is 0.3-0.4 us faster on the wave kernels)")
PDWT_TUNE(lds_fwd_batch_log2,   26, "profiles/r04za_ab_batchrange.txt",         "round 4",           "forward levels of images below 2^24 samples stay on the tiles up to 2^v")
PDWT_TUNE(lds_fwd_image_log2,   24, "profiles/r04za_ab_batchrange.txt",         "round 4",           "... images of 2^v samples and more take the wave forward there")
PDWT_TUNE(inv_wave_max_log2,    26, "profiles/r02b_wbench_b8.txt",            "round 2",           "the wave INVERSE up to 2^v samples, the LDS tiles beyond (8 x 4096^2: 224-232 vs 219 us)")
PDWT_TUNE(wave_min_columns,    512, "profiles/r04zc_small_batches.txt",       "round 4",           "images narrower than v columns never take the wave kernels (a wavefront owns 256 columns)")
PDWT_TUNE(ring_min_log2,        25, "profiles/r05c_ring_ab_batches.txt",              "round 5",           "register-ring kernels (12 / 16 taps, rows >= 1024 columns) from 2^v samples; tuning key ring_min_log2")
PDWT_TUNE(ring_min_columns,   1024, "profiles/r05c_ring_ab_batches.txt",              "round 5",           "... rows of at least v columns (512-column images lose 2x: two strips per image)")
PDWT_TUNE(long_min_taps,        18, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "strip-streaming kernels from v taps; tuning keys long_fwd / long_inv")
PDWT_TUNE(long_any_log2,        26, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "... every length from long_min_taps on from 2^v samples (db9 x 4: 172 / 193 -> 159 / 176 us)")
PDWT_TUNE(long_taps20,          20, "profiles/r06_long_ab.txt",               "round 6, 2026-10-04", "... v taps and more:")
PDWT_TUNE(long_inv_log2,        24, "profiles/r06_long_ab.txt",               "round 6, 2026-10-04", "...... the inverse from 2^v (db10 4096^2: 58.7 -> 51.3 us)")
PDWT_TUNE(long_fwd_log2,        25, "profiles/r06_long_ab.txt",               "round 6, 2026-10-04", "...... the forward from 2^v (db10 x 4: 186 -> 162 us; one image: 45 -> 49)")
PDWT_TUNE(long_fwd_mid_taps,    28, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "the forward of v taps and more already from 2^long_fwd_mid_log2 (db14 61 -> 56 us, db13 51 -> 53)")
PDWT_TUNE(long_fwd_mid_log2,    24, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "")
PDWT_TUNE(long_inv_mid_taps,    32, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "the inverse of v taps and more already from 2^long_inv_mid_log2 (db16 2048^2 level 1: 38 -> 35 us, db15 31 -> 32)")
PDWT_TUNE(long_inv_mid_log2,    22, "profiles/r06a_long_ab_thresholds.txt",   "round 6, 2026-10-04", "")
PDWT_TUNE(long_f64_fwd_max_taps,   36, "profiles/r06_f64_long_ab.txt",        "round 6, 2026-10-04", "fp64 library: the forward up to v taps (40 taps: the tap tables and the staged rows do not fit 512 registers) ...")
PDWT_TUNE(long_f64_fwd_log2,       24, "profiles/r06_f64_long_ab.txt",        "round 6, 2026-10-04", "... from 2^v samples (db13 4096^2 176 -> 118 us, db18 239 -> 200)")
PDWT_TUNE(long_f64_fwd_mid_max_taps, 32, "profiles/r06_f64_long_ab.txt",      "round 6, 2026-10-04", "... up to v taps already from 2^long_f64_min_log2 (db13 2048^2 52 -> 47 us; db18 68 -> 70)")
PDWT_TUNE(long_f64_inv_max_taps,   26, "profiles/r06_f64_long_ab.txt",        "round 6, 2026-10-04", "fp64 library: the inverse up to v taps from 2^long_f64_min_log2 (db10 4096^2 203 -> 134 us; db15 253 -> 274)")
PDWT_TUNE(long_f64_min_log2,       22, "profiles/r06_f64_long_ab.txt",        "round 6, 2026-10-04", "")
// ---- 2D DWT: tile shapes of the LDS tiles (launch_dwt2_fast.hip)
PDWT_TUNE(tile_small_level_log2, 20, "profiles/r04i_tilesweep.txt",           "round 4",           "a level below 2^v samples is one round of workgroups: small 32 x 16 / 32 x 8 tiles (40 taps 15.6 -> 7.9 us)")
PDWT_TUNE(tile_mid_hi_log2,     22, "profiles/r01c_kbench_2048.txt",          "round 1",           "levels of (2^tile_small_level_log2, 2^v] samples, <= 8 taps: the single-round 64 x 16 / 128 x 16 shapes of 512 threads")
PDWT_TUNE(pyr2_inv_big_log2,    20, "docs/LAB_NOTEBOOK.md",                   "round 2",           "inverse tile pyramid: 64 x 16 / 512 tiles from 2^v samples")
// ---- 2D DWT: several levels per launch (plan.cpp: build_schedule)
PDWT_TUNE(pyr2_max_log2,        20, "docs/LAB_NOTEBOOK.md",                   "round 1",           "tile pyramid (two levels per launch) for level pairs of at most 2^v samples")
PDWT_TUNE(pyr3_max_log2,        20, "profiles/r02y_pyr3_sweep.txt",           "round 2",           "three levels per launch: at most 2^v samples over the batch ...")
PDWT_TUNE(pyr3_image_short_log2, 20, "profiles/r05n_sched_scan.txt",        "round 5",           "... per image: 2^v when whole groups of three levels are left (haar 1024^2 L3 14.2 -> 9.1 us)")
PDWT_TUNE(pyr3_image_log2,      19, "profiles/r02y_pyr3_sweep.txt",           "round 2",           "... 2^v for filters of at most 8 taps otherwise")
PDWT_TUNE(pyr3_image_long_log2, 18, "profiles/r02y_pyr3_sweep.txt",           "round 2",           "... 2^v for 10-16 taps (sym8 512^2 L3 21.6 vs 25.0 us; 1024 x 512: 37.3 vs 25.4)")
PDWT_TUNE(inv_coarse3_above_log2, 20, "profiles/r07_inv_coarse3_ab.txt",      "round 7, 2026-10-20", "inverse only: the three coarsest levels of a large plane in one launch where it writes more than 2^v samples over the batch (up to there: the pyr3 / pyr2 rules above) ...")
PDWT_TUNE(inv_coarse3_max_log2, 22, "profiles/r07_inv_coarse3_ab.txt",        "round 7, 2026-10-20", "... and at most 2^v (the 2048^2 plane of one 4096^2 image); tuning key inv_coarse3")
PDWT_TUNE(wt_stores_max_log2,   24, "profiles/wt_stores_ab.txt",              "round 8, 2026-10-21", "write-through (sc1) 16-B stores in the inverse coarse group (11.4 -> 9.3 us) of plans of at most 2^v samples over the batch (one 4096^2 image; batches keep the L2's write combining); tuning key wt_stores")
PDWT_TUNE(wt_stores_min_log2,   22, "profiles/wt_stores_ab.txt",              "round 8, 2026-10-21", "... in the launches that write at least 2^v samples (the 2048^2 plane the coarse group of that image writes)")
PDWT_TUNE(strip2_min_log2,      26, "profiles/r01f_kbench_strip.txt",         "round 1",           "streaming strips (two forward levels per launch) from 2^v samples (8 x 4096^2: 284 -> 232 us)")
PDWT_TUNE(strip2_min_log2_haar, 25, "profiles/r04za_ab_batchrange.txt",         "round 4",           "... 2-tap filters from 2^v (8 x 2048^2 63 -> 56 us)")
PDWT_TUNE(tail_work_log2,       14, "profiles/r04zb_tailbench.txt",           "round 4",           "one-workgroup tail: planes of at most 2^v samples x taps ...")
PDWT_TUNE(tail_min_levels,       5, "profiles/r04zb_tailbench.txt",           "round 4",           "... with at least v levels left (v - 1 on planes of at most 1024 samples)")
PDWT_TUNE(tail_batch_image,   4096, "profiles/r04zc_small_batches.txt",       "round 4",           "batch mode of the tail: images of at most v samples (4096 x 64^2 db4 L3 313 -> 121 us)")
PDWT_TUNE(tail_few_batch,      384, "profiles/r04zs_tail_mid_images.txt",     "round 4",           "... images up to 4 v samples with three levels when the batch is at most v images")
PDWT_TUNE(tail_max_log2,        20, "profiles/r04zc_small_batches.txt",       "round 4",           "level-count rule of the tail below 2^v samples, batch rule from there")
// ---- 2D SWT
PDWT_TUNE(swt_fused_max_mib,   320, "profiles/r02y_bench_cfg4_batch.txt",     "round 2",           "fused 2-/4-tap SWT groups while the 3 L + 2 planes are at most v MiB (the Infinity Cache is 256)")
PDWT_TUNE(swt4_fwd_fused_odd,    1, "profiles/r06_swt4_fwd_ab.txt",           "round 6",           "... beyond that size the 4-tap FORWARD pairs stay fused (v = 1) on rows that are not whole 16-B groups: the level kernels lose 8-25 % there")
PDWT_TUNE(swt_colstream_taps,    10, "profiles/r06_swt_colstream.txt",         "round 6",           "column pass of the two-launch SWT levels streamed through an LDS history from v taps; tuning key swt_colstream")
PDWT_TUNE(swt_colstream_fwd_log2, 23, "profiles/r06_swt_colstream.txt",         "round 6",           "... the forward from 2^v samples per launch (the inverse at every size)")
PDWT_TUNE(swt_fwdstream_taps,     6, "profiles/r06_swt_fwdstream.txt",         "round 6",           "forward SWT levels (dilation 1-8) in ONE launch streamed down strips from v taps (0: never); tuning key swt_fwdstream")
PDWT_TUNE(swt_fwdstream_log2,    14, "profiles/r06_swt_fwdstream.txt",         "round 6",           "... from 2^v samples per launch")
PDWT_TUNE(swt_invstream_taps,     6, "profiles/r06_swt_invstream.txt",         "round 6",           "inverse SWT levels (dilation 1-8) in ONE launch streamed down strips from v taps (0: never); tuning key swt_invstream")
PDWT_TUNE(swt_invstream_log2,    14, "profiles/r06_swt_invstream.txt",         "round 6",           "... from 2^v samples per launch")
PDWT_TUNE(swt_invstream_max_taps, 28, "profiles/r06_swt_invstream.txt",         "round 6",           "... up to v taps (beyond: two launches, column pass on the strips)")
PDWT_TUNE(swt_invstream_f8_max_taps, 28, "profiles/r06_swt_invstream.txt",      "round 6",           "... dilation 8 up to v taps")
PDWT_TUNE(swt_tail_image,     4096, "profiles/r04zm_swt_tiny_batches.txt",    "round 4",           "whole-SWT-per-workgroup launch: images of at most v samples")
PDWT_TUNE(swt_tail_few,         64, "profiles/r04zm_swt_tiny_batches.txt",    "round 4",           "... latency mode: at most v images of at most 1024 samples with two levels and more")
PDWT_TUNE(swt_split_fwd_taps,   18, "profiles/r05k_swt_fwd_split_ab.txt",     "round 5",           "two-launch (row + column) SWT forward from v taps; tuning key swt_split_fwd")
PDWT_TUNE(swt_split_fwd_big_taps, 14, "profiles/r05k_swt_fwd_split_ab.txt",   "round 5",           "... from v taps on levels of at least 2^swt_split_fwd_big_log2 samples (sym8 2048^2 L3 160 -> 102 us)")
PDWT_TUNE(swt_split_fwd_big_log2, 21, "profiles/r05k_swt_fwd_split_ab.txt",   "round 5",           "")
PDWT_TUNE(swt_split_inv_taps,   10, "profiles/r03_swt_split_sweep.txt",       "round 3",           "two-launch SWT inverse from v taps; tuning key swt_split_inv")
PDWT_TUNE(swt_split_inv_small_taps, 24, "profiles/r05k_swt_inv_at_2p20.txt", "round 5",           "... levels of at most 2^swt_split_inv_small_log2 samples: from v taps")
PDWT_TUNE(swt_split_inv_small_log2, 20, "profiles/r05k_swt_inv_at_2p20.txt", "round 5",           "")
PDWT_TUNE(swt_split_inv_mid_taps, 12, "profiles/r03_swt_split_sweep.txt",     "round 3",           "... levels below 2^swt_split_inv_mid_log2 samples: from v taps")
PDWT_TUNE(swt_split_inv_mid_log2, 22, "profiles/r03_swt_split_sweep.txt",     "round 3",           "")
// ---- 1D DWT
PDWT_TUNE(reg1d_fwd_max_log2,   25, "profiles/r02y_bench_cfg3_batch.txt",     "round 2",           "register kernels (three levels per launch): the forward up to 2^v samples per plan")
PDWT_TUNE(reg1d_min_log2,       23, "profiles/r04v_reg1d_rows.txt",           "round 4",           "... fp32: transforms of at least 2^v samples ...")
PDWT_TUNE(reg1d_min_row,     16384, "profiles/r04v_reg1d_rows.txt",           "round 4",           "... in rows of at least v samples")
