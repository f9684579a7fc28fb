// launch.hpp -- host-side launch wrappers around the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_common.hpp"
#include "swt_kernels_args.hpp"

namespace pdwt {

// element-wise operator codes of launch_ew
enum EwOp { EW_SOFT = 0, EW_HARD = 1, EW_LINF = 2, EW_SCALE = 3 };

// threshold recipes of launch_denoise_table (== PDWT_DENOISE_BAYES / PDWT_DENOISE_VISU of pypwt_amd.h)
enum DenoiseMethod { DENOISE_BAYES = 0, DENOISE_VISU = 1 };

// The coefficient region cut into workgroup-sized pieces of ONE (band, image) pair each, for the operators that tell bands and
// images apart (ops_kernels.hpp: band_piece).  Passed by value in the kernel-argument segment.  Band b holds `batch` images
// of n[b] contiguous values from off[b] on; an image is cut into ceil(n[b] / chunk) pieces; the pieces of band b are the
// workgroups blk[b] .. blk[b + 1] - 1, image by image.
constexpr int kMaxBands = 96;
struct BandTable {
    int nbands, batch;
    long long chunk;
    long long off[kMaxBands];
    long long n[kMaxBands];
    int blk[kMaxBands + 1];
};

// Dispatch knobs that a process can move at run time (pdwt_set_tuning): the rows of tuning_knobs.inc.  A plan takes a snapshot
// when it is created and makes it the calling thread's active set around its launches, so that two threads driving plans with
// different settings -- or a third thread calling pdwt_set_tuning -- cannot change each other's kernel choice in mid-transform;
// with no active set (direct calls of the launchers: tools, emulation) the process-wide values apply.
enum class Knob : int {
#define PDWT_KNOB(key, lo, hi, init, what) key,
#include "tuning_knobs.inc"
#undef PDWT_KNOB
};
struct Tuning {
#define PDWT_KNOB(key, lo, hi, init, what) int key;
#include "tuning_knobs.inc"
#undef PDWT_KNOB
};
constexpr int kKnobCount = sizeof(Tuning) / sizeof(int);
int knob(Knob k);                         // what every launcher reads: the active snapshot's value, else the process-wide one
int set_knob(Knob k, int value);          // the process-wide value, clamped as the row says; returns the previous one
Tuning current_tuning();                  // the process-wide values now
void set_active_tuning(const Tuning* t);  // thread-local; nullptr = the process-wide values
const Tuning* active_tuning();
struct ActiveTuning {  // RAII: the plan's snapshot for the duration of a forward / inverse
    const Tuning* prev;
    explicit ActiveTuning(const Tuning* t) : prev(active_tuning()) { set_active_tuning(t); }
    ~ActiveTuning() { set_active_tuning(prev); }
};

// Which kernel FAMILY the last level launch of the calling thread went to ("tile", "wave", "ring", "generic", ...): the launch
// names of a plan (pdwt_kernel_times) say which step ran, not which of the alternative kernels served a LEVEL step; the
// dispatch-coverage test (tests/test_gpu_dispatch.py) reads this through pdwt_kernel_families.  Diagnostics only.
void note_family(const char* family);
const char* last_family();
hipError_t launch_dwt2_fwd(const Fwd2DArgs& a, int batch, hipStream_t s);
hipError_t launch_dwt2_inv(const Inv2DArgs& a, int batch, hipStream_t s);
// tuned kernels; hipErrorNotSupported = preconditions not met, use the generic launcher
hipError_t try_launch_dwt2_fwd_fast(const Fwd2DArgs& a, int batch, hipStream_t s);
hipError_t try_launch_dwt2_inv_fast(const Inv2DArgs& a, int batch, hipStream_t s);
// wave-per-tile kernels (registers + DPP, no LDS): hlen <= 8; seg_hint > 0 forces the rows per wavefront
hipError_t try_launch_dwt2_fwd_wave(const Fwd2DArgs& a, int batch, hipStream_t s, int seg_hint = 0);
hipError_t try_launch_dwt2_inv_wave(const Inv2DArgs& a, int batch, hipStream_t s, int seg_hint = 0);
// register-ring kernels for 10-20 taps (dwt2_ring_kernels.hpp): cpl = image columns per lane (4; 2 in the lab library only); seg_hint > 0
// forces the rows per wavefront
hipError_t try_launch_dwt2_fwd_ring(const Fwd2DArgs& a, int batch, hipStream_t s, int cpl = 4, int seg_hint = 0);
hipError_t try_launch_dwt2_inv_ring(const Inv2DArgs& a, int batch, hipStream_t s, int cpl = 4, int seg_hint = 0);
// strip-streaming kernels for long filters (dwt2_long_kernels.hpp): even hlen 10-40, even sides, rows of whole 16-B groups; seg_hint > 0
// forces the rows per segment
hipError_t try_launch_dwt2_fwd_long(const Fwd2DArgs& a, int batch, hipStream_t s, int seg_hint = 0);
hipError_t try_launch_dwt2_inv_long(const Inv2DArgs& a, int batch, hipStream_t s, int seg_hint = 0);
// two forward levels per wavefront (A_l stays in registers); contract of launch_dwt2_fwd_pyr2
bool dwt2_wave2_supported(int hlen, int N0r, int N0c);
hipError_t launch_dwt2_fwd_wave2(const real_t* in, real_t* const det1[3], real_t* const band2[4], int N0r, int N0c,
                                 int hlen, const FilterBank& fb, int batch, hipStream_t s, int seg_hint = 0);
// two consecutive 2D levels in one launch (small levels only, see launch_dwt2_pyramid.hip)
bool dwt2_pyramid_supported(int hlen, int N0r, int N0c, bool inverse);   // tile pyramid: even filters of at most 16 taps
bool dwt2_strip_supported(int hlen, int N0r, int N0c);     // streaming strips: at most 8 taps
hipError_t launch_dwt2_fwd_pyr2(const real_t* in, real_t* const det1[3], real_t* const band2[4], int N0r, int N0c,
                                int hlen, const FilterBank& fb, int batch, hipStream_t s);
// same contract, streaming-strip kernel for large inputs (forward only)
hipError_t launch_dwt2_fwd_strip2(const real_t* in, real_t* const det1[3], real_t* const band2[4], int N0r, int N0c,
                                  int hlen, const FilterBank& fb, int batch, hipStream_t s);
hipError_t launch_dwt2_inv_strip2(const real_t* const band2[4], const real_t* const det1[3], real_t* out, int N0r,
                                  int N0c, int hlen, const FilterBank& fb, int batch, hipStream_t s);
hipError_t launch_dwt2_inv_pyr2(const real_t* const band2[4], const real_t* const det1[3], real_t* out, int N0r, int N0c,
                                int hlen, const FilterBank& fb, int batch, hipStream_t s);
// K consecutive 2D levels in ONE launch with in-launch hand-offs between levels (dwt2_chain_kernels.hpp): (Nr, Nc) enter the
// finest level of the group; det[3 k + b] = band b (H, V, D) of the group's k-th level (finest first), app[k] its approximation
// plane (forward: outputs; inverse: app[K-1] is the input, app[K-2..0] are intermediates); flags: batch x dwt2_chain_tiles()
// zero-initialised words owned by the plan; epoch: a counter that grows with every launch on those flags
bool dwt2_chain_supported(int hlen, int Nr, int Nc, int K);
int dwt2_chain_tiles(int Nr, int Nc, int K);
hipError_t launch_dwt2_fwd_chain(const real_t* in, real_t* const* det, real_t* const* app, int Nr, int Nc, int K, int hlen,
                                 const FilterBank& fb, int batch, unsigned* flags, unsigned epoch, hipStream_t s);
hipError_t launch_dwt2_inv_chain(real_t* out, real_t* const* det, real_t* const* app, int Nr, int Nc, int K, int hlen,
                                 const FilterBank& fb, int batch, unsigned* flags, unsigned epoch, hipStream_t s);
int set_chain_timeout(int ticks);  // s_memrealtime ticks (100 MHz) a chained tile waits for a producer before computing it itself
// three consecutive 2D levels in one launch, small images (launch_dwt2_pyr3.hip): det[3 k + b] = band b (H, V, D) of the
// k-th level of the group (finest first); rows and columns multiples of 8, even filters of at most 16 taps (fp64: 8)
bool dwt2_pyr3_supported(int hlen, int N0r, int N0c);
hipError_t launch_dwt2_fwd_pyr3(const real_t* in, real_t* const det[9], real_t* out, int N0r, int N0c, int hlen,
                                const FilterBank& fb, int batch, hipStream_t s);
hipError_t launch_dwt2_inv_pyr3(const real_t* app, real_t* const det[9], real_t* out, int N0r, int N0c, int hlen,
                                const FilterBank& fb, int batch, hipStream_t s);
// the three COARSEST levels of a large plane undone in one launch (launch_dwt2_inv_coarse.hip; fp32 libraries, even filters of at
// most 8 taps): same contract as launch_dwt2_inv_pyr3; rows a multiple of 8, columns of 32, planes that hold a tile's staged regions
bool dwt2_inv_coarse3_supported(int hlen, int N0r, int N0c);
hipError_t launch_dwt2_inv_coarse3(const real_t* app, real_t* const det[9], real_t* out, int N0r, int N0c, int hlen,
                                   const FilterBank& fb, int batch, hipStream_t s);
// pdwt_set_tuning("inv_coarse3"): 0 never, 1 the size rule of build_schedule, 2 wherever supported (tests); read when a plan is built
int inv_coarse3_mode();
int set_inv_coarse3_mode(int v);  // returns the previous value
// pdwt_set_tuning("wt_stores"): whole-line write-through (sc1) stores for a launch whose output the NEXT launch reads while the plan is
// cache-resident -- the inverse coarse group of one large image (launch_dwt2.hip: wt_stores_take has the rule).  0 never, 1 the
// size rule, 2 wherever the preconditions hold (tests).  A plan keeps the value it was created with
// (pdwt_plan::wt_stores) and makes it the calling thread's active value around its launches; with no active value (direct calls of
// the launchers) the stores are plain.  fp32 libraries only.
int wt_stores_mode();
int set_wt_stores_mode(int v);       // returns the previous value
int set_wt_stores_launches(int v);   // the process-wide count of launches that took the policy: sets it, returns the previous count
void set_active_wt_stores(int mode);  // thread-local
int active_wt_stores();
struct ActiveWtStores {  // RAII, beside ActiveTuning
    int prev;
    explicit ActiveWtStores(int mode) : prev(active_wt_stores()) { set_active_wt_stores(mode); }
    ~ActiveWtStores() { set_active_wt_stores(prev); }
};
// the launcher's question: does this launch, which writes batch x (Nr, Nc) samples to `out` (images bstride elements apart), store
// write-through?  Counts the launch when it answers yes, so ask once per launch.
bool wt_stores_take(const void* out, int Nr, int Nc, long long bstride, int batch);
// ALL remaining levels of small approximations in one launch, one workgroup per image (launch_dwt2_tail.hip): (R0, C0) enter
// the group's finest level (at most 16384 samples, fp64 8192; even sizes at every level's input: powers of two or not), det[3 k + b] = band b of the
// group's k-th level (finest first); forward: in = A_{l-1}, out = A_L; inverse: in = A_L, out = A_{l-1}
bool dwt2_tail_supported(int hlen, int R0, int C0, int K);
int dwt2_tail_max_levels(int hlen, int R0, int C0, int Kmax);  // the most levels (<= Kmax) one launch can take from (R0, C0) on
hipError_t launch_dwt2_tail(const real_t* in, real_t* const* det, real_t* out, int R0, int C0, int K, int hlen, bool inverse,
                            const FilterBank& fb, int batch, hipStream_t s);
// the WHOLE 2D SWT of tiny images (at most 4096 samples, any sizes), one workgroup per image (launch_swt_tail.hip):
// det[3 (l - 1) + b] = band b of level l; forward: in = images, out = A_L; inverse: in = A_L, out = images, beta[l - 1] = the soft
// threshold applied to level l's details as they are read (nullptr: none)
bool swt2_tail_supported(int hlen, int Nr, int Nc, int L);
hipError_t launch_swt2_tail(const real_t* in, real_t* const* det, real_t* out, int Nr, int Nc, int L, int hlen, bool inverse,
                            const FilterBank& fb, const real_t* beta, int batch, hipStream_t s);
// one decimated level along the slowest axis of a volume (dwt3_axis_kernels.hpp): forward in [Nz][P] -> out [2 div2(Nz)][P] (low
// slices, then high slices); inverse the other way round (Nz = the OUTPUT's depth).  Even hlen of the built-in table; seg = steps per
// depth segment, from dwt3_depth_seg (slots = workgroups the chip keeps resident) for the width dwt3_depth_width answers: columns
// per thread, 16 B (8 B from 18 taps on) where P and both addresses allow it, else 1
int dwt3_depth_width(const void* in, const void* out, long long P, int hlen);
int dwt3_depth_steps(int Nz, int hlen, bool inverse);
int dwt3_depth_seg(int Nz, long long P, int hlen, int width, bool inverse, int slots);
int dwt3_depth_slots(int hlen, int width, bool inverse);  // resident workgroups of that kernel on the current device (occupancy x CUs)
hipError_t launch_dwt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s);
hipError_t launch_dwt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s);
// one UNDECIMATED level along the slowest axis of a volume at dilation f (swt3_axis_kernels.hpp): forward in [Nz][P] -> out [2 Nz][P]
// (low slices, then high slices); inverse the other way round.  Even hlen of the built-in table; seg = steps per segment of an orbit
// walk (swt3_depth_steps outputs per orbit), from swt3_depth_seg for the width swt3_depth_width answers
int swt3_depth_width(const void* in, const void* out, long long P, int hlen, bool inverse);
int swt3_depth_steps(int Nz, int f);
int swt3_depth_seg(int Nz, int f, long long P, int hlen, int width, int slots);
int swt3_depth_slots(int hlen, int width, bool inverse);
hipError_t launch_swt3_depth_fwd(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s);
hipError_t launch_swt3_depth_inv(const real_t* in, real_t* out, int Nz, long long P, int f, int hlen, const FilterBank& fb, int seg,
                                 hipStream_t s);
hipError_t launch_dwt1_fwd(const Fwd1DArgs& a, hipStream_t s);
hipError_t launch_dwt1_inv(const Inv1DArgs& a, hipStream_t s);
// K consecutive 1D levels in one launch (2^K must divide N0, even hlen); hipErrorNotSupported otherwise
int dwt1_fused_max_levels(int hlen);
bool dwt1_fused_supported(int hlen, int N0, int K, bool strict);  // strict: rows of 2^(K+2) samples (the several-rows-per-wavefront kernels), else 2^(K+1)
// batches of short rows: several rows per one-wavefront workgroup, any number of levels from one on (dwt1_rows_kernels.hpp)
bool dwt1_rows_tail_applies(int rows, int N0, int K, int hlen);
// up to three levels per launch in registers (dwt1_reg_kernels.hpp): even hlen <= 20, rows of >= 2048 samples
bool dwt1_reg_supported(int hlen, int N0, int K);
hipError_t launch_dwt1_fwd_reg(const real_t* in, real_t* const* det, real_t* app, int rows, int N0, int K, int hlen,
                               const FilterBank& fb, hipStream_t s);
hipError_t launch_dwt1_inv_reg(const real_t* app, const real_t* const* det, real_t* out, int rows, int N0, int K, int hlen,
                               const FilterBank& fb, hipStream_t s);
hipError_t launch_dwt1_fwd_fused(const real_t* in, real_t* const* det, real_t* app, int rows, int N0, int K, int hlen,
                                 const FilterBank& fb, hipStream_t s);
hipError_t launch_dwt1_inv_fused(const real_t* app, const real_t* const* det, real_t* out, int rows, int N0, int K,
                                 int hlen, const FilterBank& fb, hipStream_t s);
// fused a-trous level at any dilation a.f >= 1 and any (Nr, Nc): where a.f does not divide a.Nr the tiles wrap ROWS, not phase
// indices (launch_swt.hip: run_fwd / run_inv), and an index further out than one period falls back to a true modulo
// (wrap_periodic).  The stationary volume relies on both: (5, 7, 9) at level 2 is f = 2 on 7 rows, and planes below the filter length.
hipError_t launch_swt2_fwd(const Swt2DArgs& a, int batch, hipStream_t s);
hipError_t launch_swt2_inv(const Swt2DArgs& a, int batch, hipStream_t s);
bool swt2_fwd_stream_takes(const Swt2DArgs& a, int batch);  // the one-launch forward level of swt_fwdstream_kernels.hpp would take this level
hipError_t try_launch_swt2_fwd_stream(const Swt2DArgs& a, int batch, hipStream_t s);  // hipErrorNotSupported: declined
bool swt2_inv_stream_takes(const Swt2DArgs& a, int batch);
hipError_t try_launch_swt2_inv_stream(const Swt2DArgs& a, int batch, hipStream_t s);
// one a-trous level as a row launch + a column launch through scratch (2 Nr Nc batch elements): swt_split_kernels.hpp
bool swt2_split_supported(int hlen, int Nr, int Nc, int f, bool inverse, long long samples_per_launch);
hipError_t launch_swt2_split(const Swt2DArgs& a, real_t* scratch, bool inverse, int batch, hipStream_t s);
// one DECIMATED 2D level as a row launch + a column launch through scratch (Nr Nc batch elements): dwt2_split_kernels.hpp;
// (Nr, Nc) = the level's image side (forward: its input, inverse: its output), both even, Nc a multiple of 8
bool dwt2_split_supported(int hlen, int Nr, int Nc, bool inverse, long long samples_per_launch);
hipError_t launch_dwt2_split_fwd(const Fwd2DArgs& a, real_t* scratch, int batch, hipStream_t s);
hipError_t launch_dwt2_split_inv(const Inv2DArgs& a, real_t* scratch, int batch, hipStream_t s);
// levels l0 .. l0+K-1 (K = 2, 3; l0 = 1 or 4) of a 2-tap 2D SWT in one launch (swt2_fused_kernels.hpp)
bool swt2_fused_supported(int hlen, int Nr, int Nc, int l0, int K, bool inverse = false);
hipError_t launch_swt2_fused(const real_t* in, real_t* out, real_t* const* det, int Nr, int Nc, int l0, int K, bool inverse,
                             int hlen, const FilterBank& fb, const real_t* beta, int batch, hipStream_t s);
hipError_t launch_swt_pass_fwd(const SwtPassArgs& a, hipStream_t s);
hipError_t launch_swt_pass_inv(const SwtPassArgs& a, hipStream_t s);

struct NonsepArgs;
hipError_t launch_nonsep_fwd(const NonsepArgs& a, int batch, hipStream_t s);
hipError_t launch_nonsep_inv(const NonsepArgs& a, int batch, hipStream_t s);

// streaming operators over a 16-B aligned range of n floats (n % 4 == 0)
hipError_t launch_ew(int op, real_t* p, long long n, real_t b, hipStream_t s);
hipError_t launch_group_soft(real_t* d0, real_t* d1, real_t* d2, real_t* ap, long long n, real_t beta, int nb,
                             hipStream_t s);
hipError_t launch_axpy(real_t* dst, const real_t* src, long long n, real_t alpha, hipStream_t s);
hipError_t launch_norms(const real_t* p, long long n, double* scratch, double* out, hipStream_t s);  // scratch: norms_scratch_doubles() doubles; out: 2 doubles (device)
int norms_scratch_doubles();
// soft threshold + norms of the result in one sweep (ops_kernels.hpp); several sweeps share the scratch, then one final launch
hipError_t launch_soft_norms(real_t* p, long long n, long long split, real_t b_lo, real_t b_hi, bool keep_lo, bool store,
                             double* scratch, int first_block, int max_blocks, int* blocks, hipStream_t s);
hipError_t launch_norms_final(const double* scratch, int nblocks, double* out, hipStream_t s);
int norms_max_blocks();
// per (band, image) operators (ops_kernels.hpp).  partial: 2 * t.blk[t.nbands] doubles; stats: [nbands][batch][2] doubles;
// d_table: [nbands][batch] thresholds in device memory, NaN = leave that pair alone; sigma: [batch] doubles (device)
hipError_t launch_band_stats(const real_t* arena, const BandTable& t, double* partial, double* stats, hipStream_t s);
hipError_t launch_threshold_bands(int op, real_t* arena, const BandTable& t, const real_t* d_table, hipStream_t s);
hipError_t launch_denoise_table(const BandTable& t, const double* stats, const double* sigma, int method, double visu, real_t* d_table,
                                hipStream_t s);
// exact median of |c| per image by radix select (select_kernels.hpp): `passes` x (histogram sweep over band[batch][n], walk).
// state: select_state_bytes(batch) bytes and hist: select_hist_bytes(batch) bytes of device memory, both zeroed ONCE by the
// caller (the walks leave them zero again); the walk of the last pass writes sigma[image] = median / 0.6745
int select_passes();
size_t select_state_bytes(int batch);
size_t select_hist_bytes(int batch);
// (first: the images start that many values behind `band`; `band` itself stays the aligned base the 16-B groups are counted from)
hipError_t launch_select_hist(const real_t* band, long long n, int batch, int pass, void* state, unsigned* hist, hipStream_t s,
                              long long first = 0);
hipError_t launch_select_walk(long long n, int batch, int pass, int skip_zeros, void* state, unsigned* hist, double* sigma, hipStream_t s);
// the K-th largest |c| per image over the bands first_band .. of `t` (n values per image in all): the same passes with the
// histogram sweep over the pieces of `t` and a walk for the rank n - k[image].  d_k: [batch] long long in device memory;
// the last walk writes d_key[image] (select_key_bytes() each: what launch_keep_bands compares against), d_threshold[image]
// and d_kept[image].  State and histograms are those of the median select and are left zero in the same way.
size_t select_key_bytes();
hipError_t launch_select_hist_bands(const real_t* arena, const BandTable& t, int first_band, int pass, const long long* d_k,
                                    unsigned long long n, const void* state, unsigned* hist, hipStream_t s);
hipError_t launch_select_walk_rank(int batch, int pass, const long long* d_k, unsigned long long n, void* state, unsigned* hist, void* d_key,
                                   real_t* d_threshold, unsigned long long* d_kept, hipStream_t s);
// x stays iff the bit pattern of |x| >= d_key[image], else +0.0, over the bands first_band .. of `t`, in ONE launch
hipError_t launch_keep_bands(real_t* arena, const BandTable& t, int first_band, const void* d_key, hipStream_t s);
// the operators of a volume (volume_ops_kernels.hpp).  t: the swept ranges of all levels, A_L last (with_app = 0 leaves it out);
// the histogram pass and the keep sweep are the volume's counterparts of launch_select_hist_bands / launch_keep_bands for ONE
// image, to be used with launch_select_walk_rank(batch = 1).  v: the level plans' slots; stats: [1 + 7 L][2] doubles
struct VolRangeTable;
struct VolLevels;
hipError_t launch_vol_select_hist(const VolRangeTable& t, int with_app, int pass, const long long* d_k, unsigned long long n, const void* state,
                                  unsigned* hist, hipStream_t s);
hipError_t launch_vol_keep(const VolRangeTable& t, int with_app, const void* d_key, hipStream_t s);
hipError_t launch_vol_stats_reduce(const VolLevels& v, double* stats, hipStream_t s);
hipError_t launch_vol_norms(const double* stats, int nbands, double* out2, hipStream_t s);
hipError_t launch_vol_table(const VolLevels& v, const double* stats, const double* sigma, int method, double visu, real_t* d_table, hipStream_t s);
hipError_t launch_vol_expand(const VolLevels& v, const real_t* d_table, hipStream_t s);
// the group operators of a volume, all levels in ONE launch: t gives every level's member pointers and pieces; with_app: A_L is the
// eighth member at the last level.  The norm: one double per workgroup into partial[t.blk[t.nlevels]], their fixed-order sum into out[0]
struct VolGroupTable;
struct VolGroupBetas;
hipError_t launch_vol_group_soft(const VolGroupTable& t, const VolGroupBetas& betas, int with_app, hipStream_t s);
hipError_t launch_vol_group_norm(const VolGroupTable& t, int with_app, double* partial, double* out, hipStream_t s);
// circular shifts of a volume [Nz][Nr][Nc] (volume_shift_kernels.hpp), out of place: numpy.roll(in, (sz, sr, sc)) for shifts of any
// sign and size, and the weighted shift BACK into a running mean, acc = (first ? 0 : acc) + w roll(rec, (-sz, -sr, -sc))
hipError_t launch_vol_circshift(const real_t* in, real_t* out, int Nz, int Nr, int Nc, int sz, int sr, int sc, hipStream_t s);
hipError_t launch_vol_unshift_acc(const real_t* rec, real_t* acc, int Nz, int Nr, int Nc, int sz, int sr, int sc, real_t w, int first, hipStream_t s);
hipError_t launch_circshift(const real_t* in, real_t* out, int batch, int Nr, int Nc, int sr, int sc, hipStream_t s);
hipError_t launch_copy(const real_t* src, real_t* dst, long long n, hipStream_t s);  // 16-B grid-stride copy (n % 4 == 0)
hipError_t launch_fill_hash(real_t* x, long long n, uint32_t seed, real_t scale, long long index_offset,
                            hipStream_t s);

}  // namespace pdwt
