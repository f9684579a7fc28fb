/*
 * pypwt_amd.h -- C ABI of the MI355X-native wavelet transform library
 *                (libpypwt_amd.so, gfx950 HIP kernels).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference's
 * Cython module binds a C++ class directly (`cdef extern from "../pdwt/src/wt.h"`,
 * reference src/pypwt.pyx:8-61; class Wavelets, reference pdwt/src/wt.h:20-76).
 * Every method the Cython shim declares has exactly one entry point here, taking
 * an opaque handle instead of `this`; plain pointers and sizes only, no C++ or
 * torch types.  INTEGRATION.md shows the `cdef extern` block a pypwt maintainer
 * would put in place of the C++ one.
 *
 * Conventions
 *   - every function returns an int status: 0 (PDWT_OK) or a negative pdwt_status,
 *     except the getters documented as returning an element count (like the
 *     reference's get_image/get_coeff, pdwt/src/wt.cu:419-422, :473-506) and the
 *     raw-pointer getters.  pdwt_last_error() gives the message of the last
 *     failure on the calling thread.
 *   - the plan owns all device memory; host buffers belong to the caller; device
 *     pointers returned by pdwt_image_ptr / pdwt_coeff_ptr are borrowed and valid
 *     while the plan lives (pdwt/src/wt.cu:658-665).
 *   - kernels are enqueued asynchronously on the plan's HIP stream; device->host
 *     getters synchronise that stream (the reference relies on blocking
 *     cudaMemcpy on the default stream for the same effect).
 *   - plans are independent: filter taps are per plan (the reference keeps them
 *     in process-global __constant__ memory, pdwt/src/common.h:28-36), so plans
 *     with different wavelets, devices and streams can coexist.  One plan must
 *     not be used from two threads at once.
 *   - this header is the CONTRACT: what a binding of the reference's class needs.  Measurement and test hooks (per-launch
 *     timing, the level / copy micro-benchmarks, the dispatch knobs, the synthetic input) are in pypwt_amd_bench.h.
 *   - coefficient index `num` (pdwt/src/wt.cu:479-502):
 *       2D: 0 = A_L, 1 + 3(l-1) + {0,1,2} = H_l, V_l, D_l   (level 1 = finest)
 *       1D: 0 = A_L, l = D_l
 *     A batched plan (batch > 1) stores every band as [batch][rows][cols].
 */
#ifndef PYPWT_AMD_H
#define PYPWT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pdwt_plan* pdwt_handle;

/* Sample / coefficient / scalar type of the library.  libpypwt_amd.so is the fp32 build (the reference's
 * default, and the only type its Python class accepts); libpypwt_amd_f64.so is the same source built with
 * -DPDWT_DOUBLE (the reference's DOUBLEPRECISION make switch, pdwt/src/filters.h:16-30) and exports the
 * same symbols with pdwt_real = double.  Compile a client of the fp64 library with -DPDWT_DOUBLE. */
#ifdef PDWT_DOUBLE
typedef double pdwt_real;
#else
typedef float pdwt_real;
#endif

/* mirrors struct w_info (reference pdwt/src/utils.h:9-19) */
typedef struct pdwt_info {
    int ndims;   /* 1 or 2 (a 2D array with ndims == 1 is a batched 1D transform) */
    int Nr;      /* rows (1 for plain 1D) */
    int Nc;      /* columns */
    int nlevels; /* after clamping, pdwt/src/wt.cu:155-165 */
    int do_swt;  /* stationary (undecimated) transform */
    int hlen;    /* filter length */
} pdwt_info;

/* mirrors enum w_state (reference pdwt/src/wt.h:8-17) */
typedef enum pdwt_state {
    PDWT_INIT = 0,
    PDWT_FORWARD = 1,
    PDWT_INVERSE = 2,
    PDWT_THRESHOLD = 3,
    PDWT_CREATION_ERROR = 4,
    PDWT_FORWARD_ERROR = 5,
    PDWT_INVERSE_ERROR = 6,
    PDWT_THRESHOLD_ERROR = 7
} pdwt_state;

typedef enum pdwt_status {
    PDWT_OK = 0,
    PDWT_ERR_ARG = -1,          /* bad argument (null pointer, bad index, size) */
    PDWT_ERR_WAVELET = -2,      /* unknown wavelet name (reference returns -2, separable.cu:42-45) */
    PDWT_ERR_HIP = -3,          /* a HIP runtime call failed (reference -3, separable.cu:57-73) */
    PDWT_ERR_STATE = -4,        /* refused by the state machine (e.g. coefficients after inverse) */
    PDWT_ERR_FILTER_LEN = -5,   /* custom filter longer than PDWT_MAX_FILTER_WIDTH (reference -1) */
    PDWT_ERR_MISMATCH = -6,     /* add_wavelet operands differ */
    PDWT_ERR_UNSUPPORTED = -7,
    PDWT_ERR_NOMEM = -8
} pdwt_status;

#define PDWT_MAX_FILTER_WIDTH 40 /* reference pdwt/src/common.h:15 */

/* ---- construction (replaces Wavelets::Wavelets, pdwt/src/wt.cu:84-185, wt.h:42) ----
 * img: Nr*Nc pdwt_real, row-major; host memory if mem_is_on_host else device memory;
 * NULL = zero image.  Unknown wname -> PDWT_ERR_WAVELET (the reference stores -2 and
 * later hangs in w_ilog2).  levels is clamped as the reference does.
 * Uses the current HIP device and a private stream. */
int pdwt_create(const pdwt_real* img, int Nr, int Nc, const char* wname, int levels, int mem_is_on_host,
                int do_separable, int do_cycle_spinning, int do_swt, int ndim, pdwt_handle* out);

/* NEW (not in the reference): explicit device, caller stream (NULL = private stream)
 * and a batch of `batch` independent images [batch][Nr][Nc] transformed by every call. */
int pdwt_create_batched(const pdwt_real* img, int batch, int Nr, int Nc, const char* wname, int levels,
                        int mem_is_on_host, int do_separable, int do_cycle_spinning, int do_swt, int ndim,
                        int device_id, void* hip_stream, pdwt_handle* out);

/* deep copy (replaces the copy constructor, pdwt/src/wt.cu:191-222) */
int pdwt_clone(pdwt_handle src, pdwt_handle* out);
int pdwt_destroy(pdwt_handle h); /* ~Wavelets, pdwt/src/wt.cu:226-233 */

/* ---- transforms (Wavelets::forward / inverse, pdwt/src/wt.cu:236-305) ---- */
int pdwt_forward(pdwt_handle h);
int pdwt_inverse(pdwt_handle h); /* second call in a row: PDWT_ERR_STATE, nothing done */

/* ---- coefficient operators (pdwt/src/wt.cu:308-356, common.cu:219-371) ---- */
int pdwt_soft_threshold(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_hard_threshold(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_group_soft_threshold(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_shrink(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs);
int pdwt_proj_linf(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs);
int pdwt_circshift(pdwt_handle h, int sr, int sc, int inplace); /* wt.cu:364-366 */
int pdwt_norm1(pdwt_handle h, pdwt_real* out);   /* wt.cu:396-416 */
int pdwt_norm2sq(pdwt_handle h, pdwt_real* out); /* wt.cu:368-393 (1D bug at :387 not reproduced) */
/* NEW (round 6): the same two sums WITHOUT the round trip.  The results -- {sum |c|, sum c^2} as two doubles -- are written
 * to DEVICE memory on the plan's stream (d_out2, or the plan's own slot when NULL: pdwt_norms_slot) and nothing is
 * synchronised; pdwt_norm1 / pdwt_norm2sq above stay blocking host getters like the reference's (wt.cu:368-416).
 * pdwt_soft_threshold_norms_async = pdwt_soft_threshold followed by pdwt_norms_async in ONE sweep over the coefficients
 * (the inner loop of iterative shrinkage, pdwt/README.md:6-7): same arguments and state rules as pdwt_soft_threshold. */
int pdwt_norms_async(pdwt_handle h, double* d_out2);
int pdwt_norms_slot(pdwt_handle h, double** d_ptr); /* device address of the plan's own result slot (valid while the plan lives) */
int pdwt_soft_threshold_norms_async(pdwt_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize, double* d_out2);
/* ---- NEW: adaptive denoising on the device (no reference counterpart: the reference's thresholds take ONE beta for all bands,
 * wt.cu:308-325; the recipes are those of skimage.restoration.denoise_wavelet).  The threshold is picked from the data without
 * moving a coefficient to the host: every call is enqueued on the plan's stream, does not wait for it, and leaves its results
 * in device memory.  "Band" is the coefficient index `num`; "image" is an image of a batched plan (the rows of a batched 1D
 * plan are pooled, as in every other operator).  The NOISE BAND is the finest diagonal band in 2D (num 3) and the finest
 * detail band in 1D (num 1).  The small device workspace behind these calls is allocated by the first of them, so a plan
 * that never calls them keeps its footprint.
 *   pdwt_band_stats_async      {sum |c|, sum c^2} as two doubles for every (band, image), layout [nbands][batch][2], into
 *                              d_out (device memory) or the plan's own slot when NULL.  One read-only sweep, fp64
 *                              accumulation in a fixed order: bitwise reproducible from call to call.
 *   pdwt_estimate_sigma_async  sigma[image] = median(|c|) / 0.6744897501960817 over the noise band, [batch] doubles into d_out
 *                              or the plan's own slot.  The median is EXACT (a radix select on the bit pattern of |c|): the
 *                              middle element of the sorted magnitudes, or the mean in double of the two middle ones; with
 *                              skip_zeros exact zeros (-0.0 too) do not count; NaNs sort behind +inf; no element left: 0.
 *   pdwt_threshold_bands       soft (op 0) or hard (op 1) threshold, bit for bit pdwt_soft_threshold's / pdwt_hard_threshold's
 *                              arithmetic, with a threshold of its own per (band, image): table[nbands][batch] of pdwt_real in
 *                              host memory (copied on the stream through a pinned buffer) or, table_on_device != 0, in device
 *                              memory (read when the sweep runs).  A NaN entry leaves that band of that image untouched.  ONE
 *                              launch over all bands; a negative entry is accepted as a negative beta is.
 *   pdwt_denoise_async         the recipe: sigma (host memory: nsigma = 1 value for all images or nsigma = batch values; NULL =
 *                              pdwt_estimate_sigma_async), the sums, a table kernel, pdwt_threshold_bands on that table --
 *                              nothing waits for the host in between.
 *                                PDWT_DENOISE_BAYES  T[b][i] = var / sqrt(max(sumsq[b][i] / n_b - var, eps)), var = sigma[i]^2,
 *                                                    eps the machine epsilon of pdwt_real, n_b the elements of band b per image
 *                                PDWT_DENOISE_VISU   T[b][i] = sigma[i] sqrt(2 ln(Nr Nc))
 *                              computed in double and rounded once; T[0][i] (the approximation) = NaN.
 *   pdwt_adaptive_slots        device addresses of the plan's own slots (any argument may be NULL): sums [nbands][batch][2],
 *                              sigma [batch], the table of the last pdwt_denoise_async [nbands][batch]; valid while the plan
 *                              lives (read them with pdwt_copy).
 * State rules: the two read-only calls take what pdwt_norms_async takes; pdwt_threshold_bands and pdwt_denoise_async follow
 * pdwt_soft_threshold -- PDWT_ERR_STATE after pdwt_inverse, nothing done -- and, like it, do not change the plan's state.  A
 * threshold that a 2D SWT plan has deferred into its inverse is applied first, so it is seen by the sums and the median and
 * composes with the sweep; the sweep itself is always eager. */
typedef enum pdwt_denoise_method { PDWT_DENOISE_BAYES = 0, PDWT_DENOISE_VISU = 1 } pdwt_denoise_method;
int pdwt_band_stats_async(pdwt_handle h, double* d_out);
int pdwt_estimate_sigma_async(pdwt_handle h, int skip_zeros, double* d_out);
int pdwt_threshold_bands(pdwt_handle h, int op, const pdwt_real* table, int table_on_device);
int pdwt_denoise_async(pdwt_handle h, int method, int op, const double* sigma, int nsigma, int skip_zeros);
int pdwt_adaptive_slots(pdwt_handle h, double** d_stats, double** d_sigma, pdwt_real** d_table);
/* ---- NEW: best K-term approximation on the device (no reference counterpart: the reference's thresholds take a VALUE,
 * wt.cu:308-325; here the caller fixes the sparsity).  Keep the K coefficients of largest magnitude of every image and zero
 * the rest, as compression and iterative hard thresholding do.  Per image i: S = the swept bands (all detail bands, and band 0
 * when do_thresh_appcoeffs != 0), N = their elements per image, key(c) = the bit pattern of |c| (NaNs order behind +inf,
 * -0.0 == +0.0 == 0).  K[i] is clamped to [0, N].  K == 0: every element of S becomes +0.0, threshold +inf, kept 0.  K >= N:
 * nothing changes, threshold 0, kept N.  Otherwise t = the element of ascending rank N - K among the keys -- the K-th largest
 * magnitude, EXACT (the radix select of pdwt_estimate_sigma_async, over all swept bands) --; c stays, bit for bit, iff
 * key(c) >= key(t), else it becomes +0.0: ties at t all survive, kept[i] = the elements with key >= key(t) >= K (== K without
 * ties).  kept comes out of the select's walks, not out of the sweep: two calls give the same bits.  The padding behind a
 * band is neither read nor written.  "Image" is what it is to pdwt_band_stats_async (the rows of a batched 1D plan are pooled).
 * Refused with PDWT_ERR_UNSUPPORTED when N >= 2^32; the limits of the per-band operators apply.
 * State rules: pdwt_select_magnitude_async takes what pdwt_band_stats_async takes; pdwt_keep_largest_async follows
 * pdwt_threshold_bands -- PDWT_ERR_STATE after pdwt_inverse, nothing done, the plan's state unchanged.  PDWT_ERR_ARG: a null k,
 * nk not in {1, batch}, a negative K. */
/* t[i] = K[i]-th largest |c| over the swept bands of image i, kept[i] = elements with |c| >= t[i]; read-only, enqueued, no host wait.
 * k: host memory, nk = 1 (one K for all images) or nk = batch.  d_threshold [batch] pdwt_real, d_kept [batch] unsigned long long:
 * device memory, or NULL = the plan's own slots. */
int pdwt_select_magnitude_async(pdwt_handle h, const long long* k, int nk, int do_thresh_appcoeffs,
                                pdwt_real* d_threshold, unsigned long long* d_kept);
/* the select above, then ONE read-modify-write sweep over the swept bands that keeps what the rule keeps */
int pdwt_keep_largest_async(pdwt_handle h, const long long* k, int nk, int do_thresh_appcoeffs);
/* device addresses of the plan's own slots of the last of the two calls (either argument may be NULL) */
int pdwt_sparsify_slots(pdwt_handle h, pdwt_real** d_threshold, unsigned long long** d_kept);
/* dst += alpha * src ; returns 0, or the reference's codes -1..-4 / +1 (wt.cu:622-655).  On dst's stream, and ordered both ways
 * with events when the two plans have different streams, as pdwt_volume_add_wavelet is: the sum runs after what src's stream
 * holds, and what src's stream is given afterwards runs after the sum has read src.  The host waits for neither. */
int pdwt_add_wavelet(pdwt_handle dst, pdwt_handle src, pdwt_real alpha);

/* ---- data movement (pdwt/src/wt.cu:419-506) ---- */
long long pdwt_get_image(pdwt_handle h, pdwt_real* dst);          /* returns element count, <0 on error */
long long pdwt_get_coeff(pdwt_handle h, pdwt_real* dst, int num); /* 0 if refused after inverse */
/* In place: with mem_is_on_device = 1 and src == pdwt_image_ptr(h) (pdwt_coeff_ptr(h, num)) nothing is copied and the
 * host does not block -- the caller has written the buffer itself (on the plan's stream, or ordered with it by
 * pdwt_wait_for_stream) and the call only makes the image (the coefficients) current. */
int pdwt_set_image(pdwt_handle h, const pdwt_real* src, int mem_is_on_device);
int pdwt_set_coeff(pdwt_handle h, const pdwt_real* src, int num, int mem_is_on_device);
long long pdwt_coeff_count(pdwt_handle h, int num, int* rows, int* cols); /* elements incl. batch */
/* NEW: ALL coefficient bands in ONE device-to-host copy.  The reference's `coeffs` is 3 L + 1 blocking cudaMemcpy calls
 * (pypwt.pyx:287-305, wt.cu:473-506): 28 round trips for a 512^2 haar transform, which dominate its own benchmark method
 * (test/benchmark.py:141-162).  The plan keeps its bands back to back in `num` order, each padded to a multiple of 64
 * elements: pdwt_coeff_region writes the offset of every band (elements from the start of the region) into band_offsets
 * (capacity entries) and returns the region's length; pdwt_get_coeff_region copies the whole region into dst (that many
 * elements) and returns the count, 0 when refused after inverse() like pdwt_get_coeff. */
long long pdwt_coeff_region(pdwt_handle h, long long* band_offsets, int capacity);
long long pdwt_get_coeff_region(pdwt_handle h, pdwt_real* dst);
/* NEW (batched plans): one image / one image's sub-band of a batch, so that a 128-image shard can be
 * inspected without a host buffer for the whole batch; same refusal rule as pdwt_get_coeff (wt.cu:473-477) */
long long pdwt_get_image_at(pdwt_handle h, pdwt_real* dst, int image_index);
long long pdwt_get_coeff_at(pdwt_handle h, pdwt_real* dst, int num, int image_index);
intptr_t pdwt_image_ptr(pdwt_handle h);                                   /* wt.cu:658-660 */
intptr_t pdwt_coeff_ptr(pdwt_handle h, int num);                          /* wt.cu:663-665 */

/* ---- custom filter banks (pdwt/src/wt.cu:558-600) ----
 * separable plan: filter1 = low-pass, filter2 = high-pass (filter3/4 ignored)
 * non-separable : filter1..4 = LL, LH, HL, HH, each len*len row-major */
int pdwt_set_filters_forward(pdwt_handle h, const char* name, unsigned int len, const pdwt_real* filter1,
                             const pdwt_real* filter2, const pdwt_real* filter3, const pdwt_real* filter4);
int pdwt_set_filters_inverse(pdwt_handle h, const pdwt_real* filter1, const pdwt_real* filter2, const pdwt_real* filter3,
                             const pdwt_real* filter4);

/* ---- introspection ---- */
int pdwt_get_info(pdwt_handle h, pdwt_info* info, int* do_separable, int* do_cycle_spinning, int* state,
                  int* batch);
int pdwt_print_info(pdwt_handle h);                       /* print_informations, wt.cu:511-550 */
/* NEW: destroyed plans hand their device memory and stream to a small process-wide pool that new plans draw from:
 * creating + destroying a plan costs 3.4 ms of hipMalloc / hipFree / stream calls otherwise, twenty times the transform of
 * a 512^2 image (the reference's tests and tutorials build one Wavelets object per image).  Only small blocks are kept: at
 * most PDWT_POOL_BLOCK_MB (default 64 MiB) each and PDWT_POOL_MB (default 256 MiB) in total, 8 streams -- a large plan's
 * memory goes back to the driver when it is destroyed.  The library releases the pool by itself when one of its own
 * allocations fails; pdwt_trim_pool() releases everything the pool holds (call it before another allocator in the process
 * needs the memory); returns the number of blocks freed. */
int pdwt_trim_pool(void);
int pdwt_info_string(pdwt_handle h, char* buf, size_t n); /* same text into a buffer */
int pdwt_current_shift(pdwt_handle h, int* sr, int* sc);
const char* pdwt_last_error(void);
const char* pdwt_version(void);

/* ---- wavelet table ---- */
int pdwt_wavelet_count(void);
const char* pdwt_wavelet_name(int index);
/* banks: 4*hlen floats = dec_lo, dec_hi, rec_lo, rec_hi ; returns hlen or PDWT_ERR_WAVELET */
int pdwt_wavelet_filters(const char* wname, pdwt_real* banks, int capacity);

/* ---- stream / device plumbing (NEW) ---- */
int pdwt_synchronize(pdwt_handle h);
int pdwt_set_stream(pdwt_handle h, void* hip_stream); /* borrow a caller stream (e.g. torch's) */
void* pdwt_get_stream(pdwt_handle h);
int pdwt_device(pdwt_handle h);
int pdwt_device_count(void); /* HIP devices visible to the process (0: none -- every pdwt_create will fail, there is no CPU path) */
/* Ordering a DEVICE-memory source with the code that produced it (the reference runs everything on the legacy
 * default stream, so its cudaMemcpy DtoD in wt.cu:117-126,425-466 is ordered for free; a plan here owns a
 * non-blocking stream).  pdwt_set_image / pdwt_set_coeff with mem_is_on_device = 1 and pdwt_create with
 * mem_is_on_host = 0 copy on the plan's stream and return when the copy has finished (the source may then be
 * reused or freed); what they cannot know is which stream WROTE the source:
 *   pdwt_wait_for_stream(h, s)   everything submitted to the plan's stream from now on starts after the work
 *                                already submitted to stream s (NULL = the legacy default stream): an event
 *                                recorded on s and waited for on the plan's stream, the host does not block;
 *   pdwt_sync_producer(dev, s, whole_device)   host-blocking form for use before a plan exists:
 *                                hipStreamSynchronize(s), or hipDeviceSynchronize() when whole_device != 0
 *                                (the producer's stream is unknown: a __cuda_array_interface__ without "stream").
 *   pdwt_device_of_pointer(p)    the device that owns a device allocation (hipPointerGetAttributes), so that a source
 *                                with an unknown producer stream is ordered by synchronising ITS device, which need
 *                                not be the current one or the plan's; negative status for host / unknown addresses. */
int pdwt_wait_for_stream(pdwt_handle h, void* producer_stream);
int pdwt_device_of_pointer(const void* device_ptr);
int pdwt_sync_producer(int device_id, void* producer_stream, int whole_device);
/* Bind the plan's IMAGE to device memory the caller owns: from now on forward() reads its input there and inverse()
 * writes its reconstruction there (batch x Nr x Nc elements, row-major, on the plan's device; 16-byte aligned -- PDWT_ERR_ARG
 * otherwise: the tuned kernels stage the image with 16-byte accesses); pdwt_image_ptr returns it; the plan's own image buffer is
 * unused.  NULL unbinds.  pdwt_clone of a bound plan copies the image: the clone owns its copy and is not bound.  The memory must outlive the binding; nothing is copied.  Use: chaining plans without copies -- one level's
 * approximation band (pdwt_coeff_ptr(prev, 0)) IS the next level plan's image (pypwt_amd/tiled.py keeps the row slabs of an
 * image tiled over several GPUs that way).  No reference counterpart (the reference owns all its buffers, wt.cu:527-539).
 * Synchronises the plan's stream. */
int pdwt_bind_image(pdwt_handle h, void* device_ptr);
/* Copy `count` elements (of pdwt_real) between two buffers ON THE PLAN'S STREAM, ordered with its launches.  kind 0: device ->
 * device, enqueued -- the call returns at once; 1: host -> device and 2: device -> host return when the copy has finished.
 * For ROW RANGES of a plan's buffers (pdwt_image_ptr / pdwt_coeff_ptr + an offset): the slab of a rank, the halo rows of a
 * tiled image whose ring closes on the rank itself, the gathered approximation (pypwt_amd/tiled.py needs nothing else from a
 * device runtime -- no torch, no cupy).  The reference copies whole buffers only (cudaMemcpy in pdwt/src/wt.cu:425-466,470-520). */
int pdwt_copy(pdwt_handle h, void* dst, const void* src, long long count, int kind);

/* ---- NEW: neighbour exchange for ONE image tiled over several GPUs (the reference has no multi-GPU code,
 * pdwt/TODO.txt:15).  A communicator wraps an RCCL communicator (librccl is dlopen'ed on first use: single-GPU callers never
 * touch it).  One process per GPU: rank 0 calls pdwt_comm_unique_id and hands the PDWT_COMM_ID_BYTES bytes to the other
 * ranks by any means (a socket, a file, MPI: pypwt_amd/comm.py uses TCP), then every rank calls pdwt_comm_create.  All
 * transfers are enqueued on the given HIP stream -- the plan's, so that they are ordered with its level kernels -- and do
 * not block the host.  Counts are in pdwt_real values.  pdwt_comm_last_error() has the message of the last failure on the
 * calling thread; PDWT_ERR_UNSUPPORTED: librccl could not be loaded. */
typedef struct pdwt_comm* pdwt_comm_handle;
#define PDWT_COMM_ID_BYTES 128
int pdwt_comm_unique_id(void* id);
int pdwt_comm_create(const void* id, int nranks, int rank, int device_id, pdwt_comm_handle* out);
int pdwt_comm_destroy(pdwt_comm_handle c);
int pdwt_comm_rank(pdwt_comm_handle c);
int pdwt_comm_size(pdwt_comm_handle c);
/* ONE grouped point-to-point exchange (ncclGroupStart / Send / Recv / GroupEnd): message i sends send_count[i] values from
 * send_ptr[i] to rank send_peer[i] and receives recv_count[i] values into recv_ptr[i] from rank recv_peer[i]; a null
 * pointer or a zero count skips that half.  The halo rows of every band of a level are one call: neighbour traffic only
 * (xGMI links), no collective.  A rank may name itself (a ring of one: the periodic image). */
int pdwt_comm_exchange(pdwt_comm_handle c, int n, const void* const* send_ptr, const long long* send_count, const int* send_peer,
                       void* const* recv_ptr, const long long* recv_count, const int* recv_peer, void* hip_stream);
/* the two collectives of the gather step (the approximation that has become thinner than the halo goes to rank 0 and comes
 * back): recv holds size x count_per_rank values; broadcast in place from `root` */
int pdwt_comm_all_gather(pdwt_comm_handle c, const void* send, void* recv, long long count_per_rank, void* hip_stream);
int pdwt_comm_broadcast(pdwt_comm_handle c, void* buf, long long count, int root, void* hip_stream);
const char* pdwt_comm_last_error(void);

/* ---- NEW: 3D DWT of a volume [Nz][Nr][Nc] (C order).  No reference counterpart: "3D is not handled at the moment"
 * (pdwt/README.md:29), the reference's constructor stops at "ndim=%d is not implemented" (pdwt/src/wt.cu:170-172).
 * The separable decimated transform with the boundary rule of the rest of the library (an odd length is extended by repeating
 * its last sample, and that extended signal is periodic: pywt's "periodization"), one level = a depth pass along z followed by
 * one level of the batched 2D transform on the low and high slices.  div2(n) = (n + (n & 1)) / 2.
 *   - levels are clamped by the reference's rule on the SMALLEST of the three sizes (wt.cu:155-165), with its warning;
 *   - PDWT_ERR_ARG: a size below 2 on any axis, Nz > 65534 (the per-band operators take at most 65535 images, and a level
 *     holds 2 div2(Nz) of them); PDWT_ERR_WAVELET: unknown name; PDWT_ERR_UNSUPPORTED: a filter of odd length (the built-in
 *     table has none) -- all answered before any device call;
 *   - coefficient index `num`: 0 = A_L, then 1 + 7 (l - 1) + k, level 1 the finest, k over the keys of pywt.wavedecn with axes
 *     (z, y, x) in sorted order: aad, ada, add, daa, dad, dda, ddd ('a' low-pass, 'd' high-pass).  Every band is contiguous
 *     [depth][rows][cols] with (div2^l Nz, div2^l Nr, div2^l Nc) at level l;
 *   - the state machine is pdwt_state's: a second pdwt_volume_inverse in a row returns PDWT_ERR_STATE and does nothing;
 *     pdwt_volume_get_coeff answers 0 after an inverse (like pdwt_get_coeff) and the thresholds and norms PDWT_ERR_STATE,
 *     until pdwt_volume_set_coeff(num 0), pdwt_volume_set_image or pdwt_volume_forward;
 *   - soft / hard threshold: pdwt_soft_threshold's / pdwt_hard_threshold's arithmetic and arguments, bit for bit: with
 *     normalize the details of level l take beta / sqrt(2)^l and the approximation beta / sqrt(2)^L;
 *   - pdwt_volume_norms: {sum |c|, sum c^2} over all coefficients, accumulated in double; blocks;
 *   - footprint: about 3.3 volumes of device memory (the image, and per level the slice stack and its coefficients);
 *   - pointers from pdwt_volume_image_ptr / pdwt_volume_coeff_ptr are borrowed and valid while the volume lives.
 * pdwt_volume_layout is a pure host function (no device needed): the clamped level count into *nlevels, (depth, rows, cols) of
 * num 0 .. capacity - 1 into dims[3 num + {0,1,2}]; returns the number of bands 1 + 7 L, or a negative status.
 * Out of scope: 3D SWT through this constructor (pdwt_volume_create_swt below is the stationary transform), non-separable volumes, custom filter banks, clone (cycle spinning is at the end of this header; add_wavelet, shrink, the group
 * threshold and proj_linf are further down), the compiled Cython class, ShardedBatch / TiledWavelets for volumes, a fused kernel that does all three axes in
 * one read, a fused stats + threshold sweep. */
typedef struct pdwt_volume* pdwt_volume_handle;
int pdwt_volume_create(const pdwt_real* img, int Nz, int Nr, int Nc, const char* wname, int levels, int mem_is_on_host,
                       int device_id, void* hip_stream, pdwt_volume_handle* out); /* img NULL = zero volume; device_id < 0 = current; hip_stream NULL = private */
int pdwt_volume_destroy(pdwt_volume_handle h);
int pdwt_volume_forward(pdwt_volume_handle h);
int pdwt_volume_inverse(pdwt_volume_handle h);
int pdwt_volume_get_info(pdwt_volume_handle h, int* Nz, int* Nr, int* Nc, int* nlevels, int* hlen, int* state);
int pdwt_volume_layout(int Nz, int Nr, int Nc, const char* wname, int levels, int* nlevels, int* dims, int capacity);
long long pdwt_volume_get_image(pdwt_volume_handle h, pdwt_real* dst); /* returns element count, <0 on error */
int pdwt_volume_set_image(pdwt_volume_handle h, const pdwt_real* src, int mem_is_on_device);
long long pdwt_volume_get_coeff(pdwt_volume_handle h, pdwt_real* dst, int num); /* 0 if refused after inverse */
int pdwt_volume_set_coeff(pdwt_volume_handle h, const pdwt_real* src, int num, int mem_is_on_device);
long long pdwt_volume_coeff_count(pdwt_volume_handle h, int num, int* depth, int* rows, int* cols);
intptr_t pdwt_volume_image_ptr(pdwt_volume_handle h);
intptr_t pdwt_volume_coeff_ptr(pdwt_volume_handle h, int num);
int pdwt_volume_soft_threshold(pdwt_volume_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_volume_hard_threshold(pdwt_volume_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_volume_norms(pdwt_volume_handle h, double out[2]);
int pdwt_volume_synchronize(pdwt_volume_handle h);
void* pdwt_volume_stream(pdwt_volume_handle h);
/* how the depth passes of level `level` (1 .. nlevels) are launched, fixed when the volume is created: columns per thread (16 B or,
 * from 18 taps on, 8 B per lane where the plane size allows it, else 1) and the steps a workgroup walks per depth segment, forward
 * and inverse (one step = one low and one high slice forward, two output slices inverse).  Any pointer may be NULL.  Diagnostics,
 * like pdwt_schedule_string for a 2D plan. */
int pdwt_volume_depth_schedule(pdwt_volume_handle h, int level, int* width, int* seg_fwd, int* seg_inv);

/* ---- NEW: the STATIONARY (undecimated, a-trous) 3D transform of a volume: the translation-invariant transform of
 * pywt.swtn / pywt.iswtn with axes taken in the order z, y, x, the formulas of the 2D SWT of this library on every axis (analysis
 * centre hlen/2 - 1, synthesis centre hlen/2 with the factor 1/2 inside it, dilation 2^(l-1) at level l, periodic).
 * pdwt_volume_create_swt takes pdwt_volume_create's arguments and returns the same kind of handle; every pdwt_volume_* call
 * above serves it with these differences:
 *   - every band has the image's shape (Nz, Nr, Nc); numbering and keys are unchanged: 0 = A_L ('aaa' of the last level), then
 *     1 + 7 (l - 1) + k over aad .. ddd, level 1 the finest.  pywt.swtn's list is, coarsest level first, a dict per level with
 *     those seven keys and 'aaa'; the 'aaa' of a level below L is an intermediate this handle does not expose;
 *   - sizes: every axis >= 2 (any parity: the transform is periodic in the true length), Nz <= 32767 (PDWT_ERR_ARG), even
 *     filters only (PDWT_ERR_UNSUPPORTED); levels are clamped as for pdwt_volume_create;
 *   - footprint: ONE device block of (3 + 8 L) volumes -- the image, a stack of 2 Nz slices shared by all levels and four
 *     arrays of 2 Nz slices per level -- plus 256-B alignment of each buffer and a few KiB; a failed allocation returns
 *     PDWT_ERR_NOMEM and leaves nothing behind.  pdwt_volume_layout_swt is a pure host function (no device needed): the clamped
 *     level count into *nlevels and the size of that block into *device_bytes for values of sizeof_real bytes (4, 8, or 0 = this
 *     library's pdwt_real); returns the number of bands 1 + 7 L, or a negative status;
 *   - state machine, soft / hard threshold (per-level thresholds as above) and pdwt_volume_norms (A_L and the 7 L details) are
 *     the decimated volume's; sub-bands of 2^31 elements and more: the thresholds and norms return PDWT_ERR_UNSUPPORTED;
 *   - pdwt_volume_depth_schedule: columns per thread of the depth ANALYSIS (the synthesis holds twice the window and may take
 *     fewer), and the steps per segment of an orbit walk g -> (g + 2^(l-1)) mod Nz, one output slice per step and direction;
 *   - the adaptive and K-term operators below (band_stats, norms_async, estimate_sigma, threshold_bands, denoise,
 *     adaptive_slots, select_magnitude, keep_largest, sparsify_slots) return PDWT_ERR_UNSUPPORTED with a message naming the call.
 * pdwt_volume_is_swt: 1 for such a handle, 0 for a decimated volume. */
int pdwt_volume_create_swt(const pdwt_real* img, int Nz, int Nr, int Nc, const char* wname, int levels, int mem_is_on_host,
                           int device_id, void* hip_stream, pdwt_volume_handle* out);
int pdwt_volume_is_swt(pdwt_volume_handle h);
int pdwt_volume_layout_swt(int Nz, int Nr, int Nc, const char* wname, int levels, int* nlevels, long long* device_bytes, int sizeof_real);

/* The adaptive and the K-term operators (pdwt_band_stats_async ... pdwt_keep_largest_async above) on a volume.  A volume is ONE
 * image: its bands are the 1 + 7 L sub-bands in `num` order, the slices and levels of a sub-band are pooled on the device, and the
 * depth-low half of band A of every level below L -- an intermediate, not a coefficient -- is neither read nor written.  Everything
 * is enqueued on the volume's stream and nothing waits for the host (pdwt_volume_read does).
 *   - band_stats: d_out[num][2] = {sum |c|, sum c^2} of every sub-band as doubles in device memory (NULL: the volume's own slot),
 *     accumulated in double in a fixed order without float atomics: two calls give the same bits;
 *   - norms_async: d_out2[2] = the fixed-order sum of those rows (NULL: the row behind the last sub-band of the d_stats slot);
 *     pdwt_volume_norms above is unchanged;
 *   - estimate_sigma: d_out[1] = median(|ddd_1|) / 0.6744897501960817 over the WHOLE finest ddd sub-band (num 7), exact;
 *     skimage.restoration.denoise_wavelet's rule for n-D data; skip_zeros leaves exact zeros out of the median;
 *   - threshold_bands: table[num] of pdwt_real, 1 + 7 L entries in host or device memory, NaN = leave that sub-band alone, entry 0
 *     is A_L; results are bit for bit those of pdwt_volume_soft_threshold / pdwt_volume_hard_threshold with that threshold;
 *   - denoise: method and op as for pdwt_denoise_async; the BayesShrink mean is over the sub-band's elements, VisuShrink is
 *     sigma sqrt(2 ln(Nz Nr Nc)); sigma NULL = estimate it; the table (NaN at index 0) and sigma stay in the slots;
 *   - select_magnitude / keep_largest: pdwt_select_magnitude_async's rules with S = the 7 L detail sub-bands (plus A_L with
 *     do_thresh_appcoeffs) and N their element count: the key is the bit pattern of |c|, NaNs sort behind +inf, K is clamped to
 *     [0, N], K = 0 gives (+inf, 0), K >= N gives (0, N), ties with the K-th all survive, survivors stay bit for bit and the
 *     rest become +0.0.  d_threshold / d_kept: device memory, NULL = the volume's slots;
 *   - PDWT_ERR_ARG: a null handle, a negative K, a null table, an unknown op or method; PDWT_ERR_UNSUPPORTED, before anything is
 *     launched: N >= 2^32, or a noise band of that size; PDWT_ERR_STATE after pdwt_volume_inverse, with nothing done: the read-only
 *     calls as pdwt_volume_norms, the sweeps (threshold_bands, denoise, keep_largest) as the thresholds;
 *   - the slots are borrowed device pointers, valid while the volume lives, allocated by the first call that needs them;
 *     pdwt_volume_read copies `bytes` from device memory to the host on the volume's stream and waits for it. */
int pdwt_volume_band_stats_async(pdwt_volume_handle h, double* d_out);
int pdwt_volume_estimate_sigma_async(pdwt_volume_handle h, int skip_zeros, double* d_out);
int pdwt_volume_threshold_bands(pdwt_volume_handle h, int op, const pdwt_real* table, int table_on_device);
int pdwt_volume_denoise_async(pdwt_volume_handle h, int method, int op, const double* sigma, int skip_zeros);
int pdwt_volume_adaptive_slots(pdwt_volume_handle h, double** d_stats, double** d_sigma, pdwt_real** d_table);
int pdwt_volume_select_magnitude_async(pdwt_volume_handle h, long long k, int do_thresh_appcoeffs, pdwt_real* d_threshold,
                                       unsigned long long* d_kept);
int pdwt_volume_keep_largest_async(pdwt_volume_handle h, long long k, int do_thresh_appcoeffs);
int pdwt_volume_sparsify_slots(pdwt_volume_handle h, pdwt_real** d_threshold, unsigned long long** d_kept);
int pdwt_volume_norms_async(pdwt_volume_handle h, double* d_out2);
int pdwt_volume_read(pdwt_volume_handle h, void* dst, const void* d_src, long long bytes);

/* The proximal operators and the linear combination of iterative reconstruction on a volume, decimated or stationary alike.
 * A GROUP is, at level l and flat index i inside a sub-band, the seven detail sub-bands (aad[i] .. ddd[i]) -- and A_L[i] at the
 * last level with do_thresh_appcoeffs, as the reference adds c_a at the last scale (common.cu:145-170).  The depth-low half of
 * band A of a level below L (an intermediate) and padding are never a member and are never counted; nothing of these calls can be
 * seen there by a later inverse, getter or operator.
 *   - pdwt_volume_group_soft_threshold (wt.cu:329-336, common.cu:145-198, 311-341): every member becomes member * res with
 *     res = 0 if ||g||_2 = 0, else max(1 - beta_l / ||g||_2, 0), in pdwt_real; beta_l = beta, divided by sqrt 2 once per level
 *     under normalize, as for pdwt_volume_soft_threshold; the group of level L takes beta_L with or without A_L.  ONE launch;
 *   - pdwt_volume_proj_linf (wt.cu:349-356, common.cu:101-137): copysign(min(|x|, beta), x) on every detail sub-band, and on A_L
 *     with do_thresh_appcoeffs;  pdwt_volume_shrink (wt.cu:340-347, common.cu:347-371): x * (1 / (1 + beta)), the factor formed
 *     once on the host in pdwt_real; same coverage.  The Python defaults are the reference's (pypwt.pyx:406);
 *   - pdwt_volume_add_wavelet (wt.cu:622-655, common.cu:499-526): c += alpha * c_src on all 1 + 7 L sub-bands, one fused
 *     multiply-add per value, on dst's stream, ordered after what is queued on src's stream; what src's stream is given afterwards
 *     waits until the sum has read src (nothing stops the host).  Both handles must come from this
 *     library (the same pdwt_real) and agree in shape, wavelet name, levels, transform kind and device: else PDWT_ERR_MISMATCH;
 *   - pdwt_volume_group_norm (no reference counterpart; pdwt/TODO.txt:14 asks for it): *out = the sum over levels and positions of
 *     ||g||_2, the l2,1 norm whose proximal map the group threshold is.  Every term in double (the members are converted, squared
 *     and added in double, one double sqrt), the terms added in double in a fixed order without float atomics: two calls give the
 *     same bits.  No normalize.  Reads only; blocks, like pdwt_volume_norms.  pdwt_volume_group_norm_async (no reference counterpart
 *     either) leaves the result on the device and waits for nothing: in d_out[0], or in the volume's own slot when d_out is NULL; *d_slot, if given, receives the
 *     address written.  The workspace is allocated by the first of the two that is called;
 *   - PDWT_ERR_STATE after pdwt_volume_inverse, with nothing done: the four sweeps as the thresholds, the norm as
 *     pdwt_volume_norms; PDWT_ERR_UNSUPPORTED before anything is launched for a size the index math cannot hold (a stationary
 *     volume: sub-bands of 2^31 elements and more); PDWT_ERR_ARG: a null handle or a null out. */
int pdwt_volume_group_soft_threshold(pdwt_volume_handle h, pdwt_real beta, int do_thresh_appcoeffs, int normalize);
int pdwt_volume_proj_linf(pdwt_volume_handle h, pdwt_real beta, int do_thresh_appcoeffs);
int pdwt_volume_shrink(pdwt_volume_handle h, pdwt_real beta, int do_thresh_appcoeffs);
int pdwt_volume_add_wavelet(pdwt_volume_handle dst, pdwt_volume_handle src, pdwt_real alpha);
int pdwt_volume_group_norm(pdwt_volume_handle h, int do_thresh_appcoeffs, double* out);
int pdwt_volume_group_norm_async(pdwt_volume_handle h, int do_thresh_appcoeffs, double* d_out, double** d_slot);

/* Circular shifts and cycle spinning of a volume (the reference's pdwt_circshift / do_cycle_spinning, wt.cu:242-246, 303 and
 * common.cu:202-211, 378-396, exist for 2D plans only).
 *   - pdwt_volume_circshift: image <- numpy.roll(image, (sz, sr, sc)), out[z][r][c] = in[z - sz][r - sr][c - sc] with every index
 *     modulo its size: pdwt_circshift's sense on rows and columns, the same on depth.  Shifts may be negative or beyond the size.
 *     In place as the caller sees it (pdwt_volume_image_ptr does not change), on the volume's stream, decimated and stationary
 *     volumes alike; the scratch is the level-1 stack.  The image must be current -- set, or written by pdwt_volume_inverse --:
 *     after pdwt_volume_forward it returns PDWT_ERR_STATE and does nothing.  The state afterwards is that after set_image;
 *   - pdwt_volume_set_cycle_spinning(on, seed): every pdwt_volume_forward first shifts the image by a pseudo-random (sz, sr, sc),
 *     drawn on the host by a generator that depends on `seed` alone, and the matching pdwt_volume_inverse shifts the result back
 *     (Coifman and Donoho's cycle spinning, one shift per iteration of an iterative reconstruction).  Off by default: a volume
 *     that never turned it on behaves bit for bit as before.  pdwt_volume_current_shift: what the image is shifted by in all since
 *     it was set -- the last draw, or the sum of the draws of forwards in a row --, (0, 0, 0) after an inverse, after set_image and
 *     on a volume without cycle spinning.  Stationary volumes: PDWT_ERR_UNSUPPORTED (as pdwt_create refuses cycle spinning with SWT);
 *   - pdwt_volume_cycle_spin_async: the averaged estimator  image <- 1/K sum_s S_-s T^-1 theta T S_s image  over the K = nshifts
 *     shifts (sz, sr, sc) of `shifts` (host memory, read before the call returns), everything enqueued on the volume's stream.
 *     theta is, with method = PDWT_SPIN_GLOBAL, the soft (op 0) or hard (op 1) threshold with the global beta, exactly
 *     pdwt_volume_soft_threshold / _hard_threshold(beta, do_thresh_appcoeffs, normalize); with method = PDWT_DENOISE_BAYES or
 *     PDWT_DENOISE_VISU it is pdwt_volume_denoise_async(method, op, sigma, skip_zeros): with sigma NULL every shift estimates its
 *     own noise level.  The running mean has the volume's precision; the state afterwards is that after pdwt_volume_inverse.  Two
 *     extra volumes (pdwt_volume_spin_footprint tells their bytes; a pure host function, real_bytes 4, 8 or 0 = this library's) are
 *     allocated by the first call and freed with the volume; a failed allocation returns PDWT_ERR_NOMEM, leaves nothing behind
 *     and the volume usable.  Refused with nothing launched: nshifts < 1, a null `shifts`, an unknown op or method (PDWT_ERR_ARG);
 *     an image that is not current, or a volume with cycle spinning on -- the two would compose -- (PDWT_ERR_STATE); a stationary
 *     volume (PDWT_ERR_UNSUPPORTED). */
#define PDWT_SPIN_GLOBAL (-1)
int pdwt_volume_circshift(pdwt_volume_handle h, int sz, int sr, int sc);
int pdwt_volume_set_cycle_spinning(pdwt_volume_handle h, int on, unsigned long long seed);
int pdwt_volume_current_shift(pdwt_volume_handle h, int shift[3]);
int pdwt_volume_cycle_spin_async(pdwt_volume_handle h, int nshifts, const int* shifts, int op, double beta, int do_thresh_appcoeffs,
                                 int normalize, int method, const double* sigma, int skip_zeros);
int pdwt_volume_spin_footprint(int Nz, int Nr, int Nc, size_t real_bytes, size_t* extra_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PYPWT_AMD_H */
