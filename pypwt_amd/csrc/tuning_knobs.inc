// tuning_knobs.inc -- the dispatch knobs a process can move at RUN time (pdwt_set_tuning) as DATA, one row per knob:
//
//     PDWT_KNOB(key, lo, hi, initial value, "what the value decides")
//
// A plan takes a snapshot of every row when it is created and launches with it (launch.hpp: Tuning, ActiveTuning, knob()).
// launch.hpp makes the rows the fields of struct Tuning and the enumerators of Knob, launch_dwt2.hip the process-wide store,
// current_tuning() and set_knob(), plan.cpp the key names pdwt_set_tuning accepts; include/pypwt_amd_bench.h documents the
// keys for callers (tests/test_abi_cpu.py holds the two lists together).  The compile-time thresholds are tuning_gfx950.inc.
//
// pdwt_set_tuning stores 0 as it is and clamps every other value to [lo, hi] (kNoLimit: no upper limit; wave2 is a flag:
// every non-zero value, a negative one too, is 1).  The initial value is computed once, on the first use of any knob; what it
// takes from the environment (lab_env: the measurement library only) is NOT clamped.  Taps keys: the shortest filter on the
// path, 0 = never, 100 + n = n taps at every size the kernels take (tests).
#ifndef PDWT_BY_BUILD  // PDWT_BY_BUILD(fp32 libraries, fp64 library)
#ifdef PDWT_DOUBLE
#define PDWT_BY_BUILD(f32, f64) (f64)
#else
#define PDWT_BY_BUILD(f32, f64) (f32)
#endif
#endif

// ---- read by the launchers at every level launch
PDWT_KNOB(wave_min_log2, 0, 63, lab_env("PDWT_NO_WAVE") ? 63 : (lab_env("PDWT_WAVE_MIN") ? atoi(lab_env("PDWT_WAVE_MIN")) : PDWT_BY_BUILD((int)tune::wave_min_log2, (int)tune::wave_min_log2_f64)), "2D DWT levels of at least 2^v samples run on the wave-per-tile kernels (63 = never; fp64: the alternative is the generic kernel, so they start earlier)")
PDWT_KNOB(lds_max_log2,  0, 62, lab_env("PDWT_LDS_MAX") ? atoi(lab_env("PDWT_LDS_MAX")) : PDWT_BY_BUILD((int)tune::lds_max_log2, 0), "2D DWT levels of at most 2^v samples prefer the LDS tiles to the wave kernels (0 = never; fp64: no tuned LDS tiles)")
PDWT_KNOB(swt_split_fwd, 0, kNoLimit, lab_env("PDWT_SWT_SPLIT_FWD") ? atoi(lab_env("PDWT_SWT_SPLIT_FWD")) : PDWT_BY_BUILD((int)tune::swt_split_fwd_big_taps, 12), "shortest filter whose forward SWT levels run as a row launch + a column launch (swt_split_kernels.hpp; fp64: the stream kernels)")
PDWT_KNOB(swt_split_inv, 0, kNoLimit, lab_env("PDWT_SWT_SPLIT_INV") ? atoi(lab_env("PDWT_SWT_SPLIT_INV")) : PDWT_BY_BUILD((int)tune::swt_split_inv_taps, 6), "... inverse SWT levels")
PDWT_KNOB(dwt_split_fwd, 0, kNoLimit, lab_env("PDWT_DWT_SPLIT_FWD") ? atoi(lab_env("PDWT_DWT_SPLIT_FWD")) : PDWT_BY_BUILD(0, 28), "shortest filter whose forward DECIMATED 2D levels run as a row launch + a column launch (fp32: lab library only, the product keeps the value and does nothing with it; fp64: dwt2_stream_kernels.hpp)")
PDWT_KNOB(dwt_split_inv, 0, kNoLimit, lab_env("PDWT_DWT_SPLIT_INV") ? atoi(lab_env("PDWT_DWT_SPLIT_INV")) : PDWT_BY_BUILD(0, 28), "... inverse levels")
PDWT_KNOB(ring_min_log2, 0, 63, (int)tune::ring_min_log2, "2D DWT levels of at least 2^v samples with 12 / 16 taps run on the register-ring kernels (63 = never; below the default: 10-20 taps, any width -- tests)")
PDWT_KNOB(long_fwd,      0, kNoLimit, (int)tune::long_min_taps, "shortest filter whose large forward 2D DWT levels run on the strip-streaming kernels (dwt2_long_kernels.hpp)")
PDWT_KNOB(long_inv,      0, kNoLimit, (int)tune::long_min_taps, "... inverse levels")
PDWT_KNOB(swt_colstream, 0, kNoLimit, (int)tune::swt_colstream_taps, "shortest filter whose two-launch SWT levels stream their column pass through an LDS history (swt_colstream_kernels.hpp)")
PDWT_KNOB(swt_fwdstream, 0, kNoLimit, (int)tune::swt_fwdstream_taps, "shortest filter whose forward SWT levels run in one launch (swt_fwdstream_kernels.hpp)")
PDWT_KNOB(swt_invstream, 0, kNoLimit, (int)tune::swt_invstream_taps, "... inverse SWT levels (swt_invstream_kernels.hpp)")
// ---- read by build_schedule when a plan is built: a clone rebuilds its launch lists from its source's values
PDWT_KNOB(wave2,         1, 1,  lab_env("PDWT_WAVE2") ? 1 : 0, "two forward levels per wavefront (opt-in)")
PDWT_KNOB(swt_fused,     0, 2,  lab_env("PDWT_SWT_FUSED") ? atoi(lab_env("PDWT_SWT_FUSED")) : 1, "2-tap 2D SWT levels 1-3 / 4-6 and 4-tap pairs in one launch each (swt2_fused_kernels.hpp); 2: beyond the cache-size limit too")
PDWT_KNOB(chain,         0, 3,  lab_env("PDWT_CHAIN") ? atoi(lab_env("PDWT_CHAIN")) : 0, "levels chained inside one launch: 0 never (opt-in: measured no faster, and the product stubs the kernels out), 1 one cache-resident image + batch inverses, 2 wherever supported (tests), 3 = 2 + batch forwards")
PDWT_KNOB(reg1d,         0, 15, lab_env("PDWT_REG1D") ? (atoi(lab_env("PDWT_REG1D")) & 15) : 3, "1D levels three at a time in registers (dwt1_reg_kernels.hpp): bit 0 forward, bit 1 inverse, bits 2 / 3 lift the size limits")
// ---- beside the table, like chain_timeout: "inv_coarse3" (0, 2; initially 1; PDWT_INV_COARSE3 in the measurement library) -- the inverse of
// the three coarsest levels of a large plane in one launch (dwt2_inv_coarse_kernels.hpp): 0 never, 1 the size rule of build_schedule,
// 2 wherever the kernel applies (tests).  The rows above are pinned one by one to the setters they replaced (tests/test_abi_cpu.py:
// KNOB_RECORD, sixteen rows), so a key that never had such a setter lives in launch_dwt2_inv_coarse.hip (set_inv_coarse3_mode) and in
// the plan (pdwt_plan::inv_coarse3: a clone rebuilds its launch lists from its source's value).
// "wt_stores" (0, 2; initially 1; PDWT_WT_STORES in the measurement library) is kept the same way (launch_dwt2.hip: set_wt_stores_mode,
// pdwt_plan::wt_stores): 16-B write-through stores in the inverse coarse group -- 0 never, 1 in plans of at most 2^wt_stores_max_log2
// samples where the launch writes at least 2^wt_stores_min_log2 (tuning_gfx950.inc), 2 wherever the stores' preconditions hold
// (tests).  "wt_stores_launches" reads (and sets) the process-wide count of launches that took it: not a dispatch key.
