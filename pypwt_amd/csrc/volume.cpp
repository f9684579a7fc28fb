// volume.cpp -- the pdwt_volume_* block of the C ABI (include/pypwt_amd.h).  A handle is one of two objects (volume.hpp):
//   pdwt::VolumeDwt  the 3D DWT as depth passes (launch_depth3.hip) around one-level batched 2D plans.  The 2D side goes through the
//                    plans' own entry points -- pdwt_create_batched, pdwt_forward / pdwt_inverse, pdwt_threshold_bands,
//                    pdwt_band_stats_async --, so nothing a 1D or 2D plan does is restated here.  The adaptive and K-term operators
//                    pool the slices and levels of a sub-band on the device (volume_ops_kernels.hpp, launch_volume_ops.hip): a
//                    volume is ONE image.
//   pdwt::VolumeSwt  the stationary transform: no level plans, a-trous depth passes (launch_depth3.hip) around the batched 2D SWT
//                    launchers of launch.hpp, called directly, on one device block.
// The entry points at the end check their arguments and the state, select the device and call the object.
#include "volume.hpp"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <strings.h>

#include <limits>

#include "host_util.hpp"
#include "launch.hpp"
#include "wavelet_table.hpp"

using namespace pdwt;

namespace {

#define VFAIL(code, ...) set_last_error((code), __VA_ARGS__)

// the seven detail sub-bands of a level in pywt.wavedecn's sorted key order, axes (z, y, x): depth half (0 low, 1 high) and
// band of the level's 2D plan (0 A, 1 H, 2 V, 3 D)
const struct { const char* key; int half, band; } kSub[7] = {
    {"aad", 0, 2}, {"ada", 0, 1}, {"add", 0, 3}, {"daa", 1, 0}, {"dad", 1, 2}, {"dda", 1, 1}, {"ddd", 1, 3}};

// the per-band operators of a batched plan take at most 65535 images, and a level's plan holds 2 div2(Nz) of them
constexpr int kMaxDepthDwt = 65534;
// the batched 2D level of a stationary volume runs 2 Nz planes in gridDim.z
constexpr int kMaxDepthSwt = 32767;

// argument checks shared by the creates and the layouts; no HIP call
int check_shape(const char* what, int Nz, int Nr, int Nc, const char* wname, int max_depth, const WaveletEntry** w) {
    if (Nz < 2 || Nr < 2 || Nc < 2) return VFAIL(PDWT_ERR_ARG, "%s: every axis needs at least 2 samples, got (%d, %d, %d)", what, Nz, Nr, Nc);
    if (Nz > max_depth) return VFAIL(PDWT_ERR_ARG, "%s: depth %d is beyond the limit of %d slices", what, Nz, max_depth);
    if (!wname) return VFAIL(PDWT_ERR_ARG, "%s: wname is null", what);
    *w = find_wavelet(wname);
    if (!*w) return VFAIL(PDWT_ERR_WAVELET, "unknown wavelet name %s", wname);
    if ((*w)->hlen & 1) return VFAIL(PDWT_ERR_UNSUPPORTED, "%s: filters of odd length are not built for volumes", what);
    return PDWT_OK;
}

// the reference's clamp (wt.cu:155-165) on the smallest of the three sizes; what the rule leaves is treated as pdwt_create does
int clamp_levels(int Nz, int Nr, int Nc, const char* wname, int hlen, int levels, bool warn) {
    if (levels < 1) {
        if (warn) puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        levels = 1;
    }
    const int N = Nz < Nr ? (Nz < Nc ? Nz : Nc) : (Nr < Nc ? Nr : Nc);
    int wmaxlev = ilog2(N / (hlen - 1));
    if (wmaxlev < 1) wmaxlev = 1;
    if (levels > wmaxlev) {
        if (warn) {
            printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on a %dx%dx%d volume.\n",
                   levels, wname, wmaxlev, Nc, Nr, Nz);
            printf("Forcing nlevels = %d\n", wmaxlev);
        }
        levels = wmaxlev;
    }
    return levels;
}

template <typename T>  // double (the wavelet table) or real_t (a caller's bank)
void fill_bank(pdwt_volume* v, int hlen, const T* dec_lo, const T* dec_hi, const T* rec_lo, const T* rec_hi) {
    for (int i = 0; i < kMaxTaps; i++) {
        const bool in = i < hlen;
        v->dec.lo[i] = in ? (real_t)dec_lo[i] : 0, v->dec.hi[i] = in ? (real_t)dec_hi[i] : 0;
        v->rec.lo[i] = in ? (real_t)rec_lo[i] : 0, v->rec.hi[i] = in ? (real_t)rec_hi[i] : 0;
    }
}

// What both creates do first: the checks that need no device, the device, and a new V that knows its sizes, its levels, its name
// and its bank and owns nothing yet.  device_id < 0 becomes the current device.
template <class V>
int open_volume(const char* what, int Nz, int Nr, int Nc, const char* wname, int levels, int max_depth, int& device_id,
                pdwt_volume_handle* out, V** made) {
    if (!out) return VFAIL(PDWT_ERR_ARG, "%s: out is null", what);
    *out = nullptr;
    const WaveletEntry* w = nullptr;
    PDWT_TRY(check_shape(what, Nz, Nr, Nc, wname, max_depth, &w));

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return VFAIL(PDWT_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device_id < 0) HIP_TRY(hipGetDevice(&device_id));
    if (device_id >= ndev) return VFAIL(PDWT_ERR_ARG, "device %d out of range (%d devices)", device_id, ndev);

    V* v = new V();
    v->device = device_id;
    v->Nz = Nz, v->Nr = Nr, v->Nc = Nc;
    v->hlen = w->hlen;
    v->nlevels = clamp_levels(Nz, Nr, Nc, wname, w->hlen, levels, true);
    snprintf(v->wname, sizeof(v->wname), "%s", wname);
    fill_bank(v, w->hlen, w->dec_lo, w->dec_hi, w->rec_lo, w->rec_hi);
    *made = v;
    return PDWT_OK;
}

// the image a create was given (or zeros), on the volume's stream
hipError_t upload_image(pdwt_volume* v, const pdwt_real* img, int mem_is_on_host) {
    const size_t bytes = (size_t)v->Nz * v->Nr * v->Nc * sizeof(real_t);
    hipError_t e = img ? hipMemcpyAsync(v->image, img, bytes, mem_is_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, v->stream)
                       : hipMemsetAsync(v->image, 0, bytes, v->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(v->stream);
    return e;
}

int num_bands(const pdwt_volume* v) { return 1 + 7 * v->nlevels; }

bool locate(const pdwt_volume* v, int num, SubBand* s) {
    if (num < 0 || num >= num_bands(v)) return false;
    if (num == 0) {
        s->level = v->nlevels;
        s->half = 0;
        s->band = 0;
    } else {
        s->level = (num - 1) / 7 + 1;
        s->half = kSub[(num - 1) % 7].half;
        s->band = kSub[(num - 1) % 7].band;
    }
    s->depth = v->nz[s->level];
    s->rows = v->nr[s->level];
    s->cols = v->nc[s->level];
    return true;
}

const real_t kLeave = std::numeric_limits<real_t>::quiet_NaN();  // a NaN entry of a threshold table leaves that (band, image) alone

// The thresholds of the global soft / hard threshold: b[l - 1] for the details of level l = 1 .. L -- beta, divided by sqrt 2 once
// per level under `normalize` (plan.cpp: threshold_sweep, common.cu:244) -- and, returned, the one of A_L (kLeave when do_app is 0).
real_t level_thresholds(real_t beta, int L, int do_app, int normalize, std::vector<real_t>* b) {
    b->resize(L);
    real_t x = beta;
    for (int l = 1; l <= L; l++) {
        if (normalize > 0) x = (real_t)(x / 1.4142135623730951);
        (*b)[l - 1] = x;
    }
    return do_app ? app_beta(beta, L, normalize) : kLeave;
}

// The two norms from the sums (sum |c|, sum c^2) of every (level, band, image): all details, and the depth-low half of band A at
// the last level only, in a fixed order -- levels ascending, bands A H V D, the 2 half[l] images of a band in index order (the
// depth-low half first) --, in double.  term(l, b, i) points at the two sums of image i of band b of level l.
template <class Term>
void sum_norms(int L, const int* half, Term term, double out[2]) {
    double n1 = 0, n2 = 0;
    for (int l = 1; l <= L; l++)
        for (int b = 0; b < 4; b++)
            for (int i = 0; i < 2 * half[l]; i++) {
                if (b == 0 && i < half[l] && l != L) continue;
                const double* s = term(l, b, i);
                n1 += s[0];
                n2 += s[1];
            }
    out[0] = n1, out[1] = n2;
}

// ---------------------------------------------------------------- operators that pool slices and levels (volume_ops_kernels.hpp)

// every level's plan is told that its coefficients are current: they were written in place (pypwt_amd/tiled.py:431-437)
int mark_current(VolumeDwt* v) {
    for (pdwt_handle p : v->plans) PDWT_TRY(pdwt_set_coeff(p, reinterpret_cast<const real_t*>(pdwt_coeff_ptr(p, 0)), 0, 1));
    return PDWT_OK;
}

// the swept ranges of the K-term operators: per level bands H, V, D and the depth-high half of band A, then A_L; no HIP call
void build_ranges(VolumeDwt* v) {
    const int L = v->nlevels;
    for (int which = 0; which < 2; which++) {
        VolRangeTable& t = which ? v->rt_keep : v->rt_hist;
        t.nranges = 0;
        for (int l = 1; l <= L; l++) {
            const pdwt_plan* p = v->plans[l - 1];
            const long long off[4] = {p->bands[0].off, p->bands[1].off, p->bands[2].off, p->bands[3].off};
            vol_ranges_add_level(t, p->arena, off, v->nz[l], (long long)v->nr[l] * v->nc[l]);
        }
        // the pieces of select_hist_bands_kernel (about 1024 of 8192 values at least) and of keep_bands_kernel (2048, 4096): plan.cpp
        const pdwt_plan* p = v->plans[L - 1];
        const long long all = vol_ranges_finish(t, p->arena, p->bands[0].off, v->nz[L], (long long)v->nr[L] * v->nc[L], which ? 2048 : 1024,
                                                which ? 4096 : 8192);
        v->n_app = (unsigned long long)v->nz[L] * v->nr[L] * v->nc[L];
        v->n_details = (unsigned long long)all - v->n_app;
    }
}

void free_ops(VolumeWs* w) {
    if (w->block) (void)hipFree(w->block);
    if (w->h_stage) (void)hipHostFree(w->h_stage);
    if (w->staged) (void)hipEventDestroy(w->staged);
    delete w;
}

int ensure_ops(VolumeDwt* v) {
    if (v->ops) return PDWT_OK;
    const int nb = num_bands(v), L = v->nlevels;
    VolumeWs* w = new VolumeWs();
    // (the two sums over all coefficients sit behind the last sub-band's row)
    const size_t sz_stats = align256((size_t)2 * (nb + 1) * sizeof(double)), sz_sigma = 256, sz_table = align256((size_t)nb * sizeof(real_t)),
                 sz_state = align256(select_state_bytes(1)), sz_hist = align256(select_hist_bytes(1)), sz_one = 256,
                 sz_all = sz_stats + sz_sigma + sz_table + sz_state + sz_hist + 4 * sz_one;
    hipError_t e = hipMalloc(&w->block, sz_all);
    if (e == hipSuccess) e = hipMemsetAsync(w->block, 0, sz_all, v->stream);  // the walks leave state and histogram zero again
    if (e == hipSuccess) e = hipHostMalloc(&w->h_stage, 16, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&w->staged, hipEventDisableTiming);
    int rc = e == hipSuccess ? PDWT_OK : VFAIL(PDWT_ERR_HIP, "workspace of the volume's operators: %s", hipGetErrorString(e));
    VolLevels& lv = w->levels;
    lv.nlevels = L;
    lv.entry[0] = 0;
    for (int l = 1; l <= L && rc == PDWT_OK; l++) {
        double* d_stats = nullptr;
        real_t* d_table = nullptr;
        rc = pdwt_adaptive_slots(v->plans[l - 1], &d_stats, nullptr, &d_table);
        lv.half[l - 1] = v->nz[l];
        lv.n[l - 1] = (long long)v->nz[l] * v->nr[l] * v->nc[l];
        lv.stats[l - 1] = d_stats;
        lv.table[l - 1] = d_table;
        lv.entry[l] = lv.entry[l - 1] + 4 * 2 * v->nz[l];
    }
    if (rc != PDWT_OK) {
        (void)hipGetLastError();
        free_ops(w);
        return rc;
    }
    char* at = static_cast<char*>(w->block);
    auto take = [&](size_t bytes) {
        char* here = at;
        at += bytes;
        return here;
    };
    w->stats = reinterpret_cast<double*>(take(sz_stats));
    w->norms = w->stats + 2 * nb;
    w->sigma = reinterpret_cast<double*>(take(sz_sigma));
    w->table = reinterpret_cast<real_t*>(take(sz_table));
    w->sel_state = take(sz_state);
    w->sel_hist = reinterpret_cast<unsigned*>(take(sz_hist));
    w->sp_k = reinterpret_cast<long long*>(take(sz_one));
    w->sp_key = take(sz_one);
    w->sp_threshold = reinterpret_cast<real_t*>(take(sz_one));
    w->sp_kept = reinterpret_cast<unsigned long long*>(take(sz_one));
    v->ops = w;
    return PDWT_OK;
}

// at most 8 bytes of host data (K, a noise level) to device memory on the volume's stream through the pinned staging buffer; the
// host waits only if the previous upload has not left the buffer yet (as plan.cpp's stage_upload does for a plan)
int stage_upload(VolumeDwt* v, void* d_dst, const void* h_src, size_t bytes) {
    VolumeWs* w = v->ops;
    HIP_TRY(hipEventSynchronize(w->staged));
    memcpy(w->h_stage, h_src, bytes);
    HIP_TRY(hipMemcpyAsync(d_dst, w->h_stage, bytes, hipMemcpyHostToDevice, v->stream));
    HIP_TRY(hipEventRecord(w->staged, v->stream));
    return PDWT_OK;
}

// The decimated object behind a handle, for the operator entry points; a stationary volume has none of them yet.
int as_dwt(pdwt_volume_handle v, const char* what, VolumeDwt** d) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->do_swt)
        return VFAIL(PDWT_ERR_UNSUPPORTED, "%s: the adaptive and K-term operators are not built for stationary volumes (do_swt)", what);
    *d = static_cast<VolumeDwt*>(v);
    return PDWT_OK;
}

// What every operator does first.  The read-only ones take what pdwt_volume_norms takes; the sweeps follow the thresholds.
int enter_ops(VolumeDwt* v, const char* what, bool sweep) {
    if (v->state == PDWT_INVERSE)
        return sweep ? VFAIL(PDWT_ERR_STATE, "%s: cannot threshold coefficients, as they were modified by inverse()", what)
                     : VFAIL(PDWT_ERR_STATE, "%s: the coefficients were modified by inverse()", what);
    PDWT_TRY(mark_current(v));
    return ensure_ops(v);
}

// per-slice sums by every level's plan, then one wavefront per sub-band adds up the slices of its depth half
int band_stats_impl(VolumeDwt* v, double* d_out) {
    for (pdwt_handle p : v->plans) PDWT_TRY(pdwt_band_stats_async(p, nullptr));
    HIP_TRY(launch_vol_stats_reduce(v->ops->levels, d_out ? d_out : v->ops->stats, v->stream));
    return PDWT_OK;
}

// the exact median of |ddd_1|: the depth-high half of band D of level 1's plan is one contiguous image, `first` values into the arena
int noise_check(const pdwt_volume* v, const char* what) {
    const long long n = (long long)v->nz[1] * v->nr[1] * v->nc[1];
    return n >= (1LL << 32) ? VFAIL(PDWT_ERR_UNSUPPORTED, "%s: the noise band has %lld elements (the histogram bins are 32-bit)", what, n) : PDWT_OK;
}

int estimate_sigma_impl(VolumeDwt* v, int skip_zeros, double* d_out) {
    VolumeWs* w = v->ops;
    const pdwt_plan* p = v->plans[0];
    const long long n = (long long)v->nz[1] * v->nr[1] * v->nc[1];
    for (int pass = 0; pass < select_passes(); pass++) {
        HIP_TRY(launch_select_hist(p->arena, n, 1, pass, w->sel_state, w->sel_hist, v->stream, p->bands[3].off + n));
        HIP_TRY(launch_select_walk(n, 1, pass, skip_zeros ? 1 : 0, w->sel_state, w->sel_hist, d_out ? d_out : w->sigma, v->stream));
    }
    return PDWT_OK;
}

// every level's sweep with the table its plan holds in its own slot
int sweep_levels(VolumeDwt* v, int op) {
    for (int l = 1; l <= v->nlevels; l++) PDWT_TRY(pdwt_threshold_bands(v->plans[l - 1], op, v->ops->levels.table[l - 1], 1));
    return PDWT_OK;
}

// N: the swept elements; refused before anything is launched when the 32-bit histogram bins could overflow
unsigned long long swept(const VolumeDwt* v, int do_app) { return v->n_details + (do_app ? v->n_app : 0); }

int sparsify_check(const VolumeDwt* v, const char* what, long long k, int do_app) {
    if (k < 0) return VFAIL(PDWT_ERR_ARG, "%s: K = %lld is negative", what, k);
    if (swept(v, do_app) >= (1ULL << 32))
        return VFAIL(PDWT_ERR_UNSUPPORTED, "%s: %llu swept elements (the histogram bins are 32-bit)", what, swept(v, do_app));
    return PDWT_OK;
}

// the K-th largest |c| over the detail sub-bands (and A_L): the passes of plan.cpp's select_magnitude_impl for ONE image whose
// pieces lie in every level's arena
int select_magnitude_impl(VolumeDwt* v, long long k, int do_app, real_t* d_threshold, unsigned long long* d_kept) {
    VolumeWs* w = v->ops;
    const unsigned long long n = swept(v, do_app);
    PDWT_TRY(stage_upload(v, w->sp_k, &k, sizeof(k)));
    for (int pass = 0; pass < select_passes(); pass++) {
        HIP_TRY(launch_vol_select_hist(v->rt_hist, do_app ? 1 : 0, pass, w->sp_k, n, w->sel_state, w->sel_hist, v->stream));
        HIP_TRY(launch_select_walk_rank(1, pass, w->sp_k, n, w->sel_state, w->sel_hist, w->sp_key, d_threshold ? d_threshold : w->sp_threshold,
                                        d_kept ? d_kept : w->sp_kept, v->stream));
    }
    return PDWT_OK;
}

// The table of the group operators: per level the seven detail sub-bands in key order and, at the last level, A_L, as pointers
// into the level's four band arrays (sub_ptr of the depth-low half is the array's start), and the pieces: about 2048 workgroups over
// all levels, 2048 positions (14 K values) at least each.  No HIP call.
void build_groups(pdwt_volume* v) {
    VolGroupTable& t = v->groups;
    t.nlevels = 0;
    for (int l = 1; l <= v->nlevels; l++) {
        real_t* band[4];
        for (int b = 0; b < 4; b++) band[b] = v->sub_ptr(SubBand{l, 0, b, v->nz[l], v->nr[l], v->nc[l]});
        vol_group_add_level(t, band, (long long)v->nz[l] * v->nr[l] * v->nc[l], l == v->nlevels);
    }
    vol_group_finish(t, 2048, 2048);
}

// the workspace of group_norm: the result slot and one partial sum per piece
int ensure_group_ws(pdwt_volume* v) {
    if (v->group_ws) return PDWT_OK;
    const size_t bytes = align256((size_t)(1 + v->groups.blk[v->groups.nlevels]) * sizeof(double));
    const hipError_t e = hipMalloc((void**)&v->group_ws, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        v->group_ws = nullptr;
        return VFAIL(PDWT_ERR_NOMEM, "workspace of group_norm: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    return PDWT_OK;
}

// the one device block of a stationary volume, in bytes from its start (volume.hpp has the picture); no HIP call
struct SwtLayout {
    size_t image = 0, stack = 0, bands = 0, band = 0, stats = 0, partial = 0, table = 0, total = 0;
    long long chunk = 0;
    int pieces = 0;
};

SwtLayout swt_layout(int Nz, int Nr, int Nc, int L, size_t real_bytes) {
    SwtLayout y;
    const long long n = (long long)Nz * Nr * Nc;  // one volume = one depth half of a band array
    const size_t vol = align256((size_t)n * real_bytes);
    y.band = align256((size_t)2 * n * real_bytes);
    y.image = 0;
    y.stack = vol;
    y.bands = y.stack + y.band;
    // sweep geometry of ONE level (threshold and sums alike): about 1024 pieces of at least 4096 values, each inside one half
    y.chunk = ((8 * n + 1023) / 1024 + 1023) / 1024 * 1024;
    if (y.chunk < 4096) y.chunk = 4096;
    y.pieces = (int)(8 * ((n + y.chunk - 1) / y.chunk));
    y.stats = y.bands + (size_t)4 * L * y.band;
    y.partial = y.stats + align256((size_t)L * 16 * sizeof(double));
    y.table = y.partial + align256((size_t)L * 2 * y.pieces * sizeof(double));
    y.total = y.table + align256((size_t)L * 8 * real_bytes) + 256;  // slack: the one-launch 2D kernels may read 12 B past a plane
    return y;
}


// ---------------------------------------------------------------- circular shifts and cycle spinning (volume_shift_kernels.hpp)

// the image is what the caller last gave or the last inverse wrote; after a forward it is the transform's input and the level-1
// stack holds live data
bool image_current(const pdwt_volume* v) { return v->state == PDWT_INIT || v->state == PDWT_INVERSE; }

// image <- circshift(image, sz, sr, sc) through the level-1 stack: shifted into it, copied back, so that the image stays where it is
int shift_image(pdwt_volume* v, int sz, int sr, int sc) {
    if (!vol_shift_reduce(sz, v->Nz) && !vol_shift_reduce(sr, v->Nr) && !vol_shift_reduce(sc, v->Nc)) return PDWT_OK;
    real_t* tmp = v->shift_scratch();
    HIP_TRY(launch_vol_circshift(v->image, tmp, v->Nz, v->Nr, v->Nc, sz, sr, sc, v->stream));
    return v->copy(v->image, tmp, (long long)v->Nz * v->Nr * v->Nc, 0);
}

// splitmix64: the draws of a cycle-spinning volume depend on its seed alone
unsigned long long spin_draw(pdwt_volume* v) {
    unsigned long long z = (v->rng += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

size_t spin_volume_bytes(int Nz, int Nr, int Nc, size_t real_bytes) { return align256((size_t)Nz * Nr * Nc * real_bytes); }

// the kept source and the running mean of cycle_spin: one block, or nothing
int ensure_spin(pdwt_volume* v) {
    if (v->spin_block) return PDWT_OK;
    const size_t vol = spin_volume_bytes(v->Nz, v->Nr, v->Nc, sizeof(real_t));
    const hipError_t e = hipMalloc(&v->spin_block, 2 * vol);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        v->spin_block = nullptr;
        return VFAIL(PDWT_ERR_NOMEM, "cycle_spin: hipMalloc of %zu bytes failed: %s", 2 * vol, hipGetErrorString(e));
    }
    v->spin_src = static_cast<real_t*>(v->spin_block);
    v->spin_acc = reinterpret_cast<real_t*>(static_cast<char*>(v->spin_block) + vol);
    return PDWT_OK;
}

// the sweep of pdwt_volume_denoise_async on current coefficients: the noise level is in its slot already, or is estimated
int denoise_sweep(VolumeDwt* v, int method, int op, bool estimate, int skip_zeros) {
    VolumeWs* w = v->ops;
    if (estimate) PDWT_TRY(estimate_sigma_impl(v, skip_zeros, nullptr));
    if (method == PDWT_DENOISE_BAYES) PDWT_TRY(band_stats_impl(v, nullptr));
    const double visu = sqrt(2.0 * log((double)v->Nz * (double)v->Nr * (double)v->Nc));
    HIP_TRY(launch_vol_table(w->levels, w->stats, w->sigma, method, visu, w->table, v->stream));
    HIP_TRY(launch_vol_expand(w->levels, w->table, v->stream));
    return sweep_levels(v, op);
}

}  // namespace

// ---------------------------------------------------------------- the common part
int pdwt_volume::set_filters(int n, const real_t* dec_lo, const real_t* dec_hi, const real_t* rec_lo, const real_t* rec_hi) {
    fill_bank(this, n, dec_lo, dec_hi, rec_lo, rec_hi);
    return PDWT_OK;
}

// ---------------------------------------------------------------- the decimated volume
namespace pdwt {

VolumeDwt::~VolumeDwt() {
    if (!plans.empty()) (void)hipStreamSynchronize(stream);
    if (ops) free_ops(ops);
    if (group_ws) (void)hipFree(group_ws);
    if (spin_block) (void)hipFree(spin_block);
    for (size_t i = plans.size(); i-- > 0;) pdwt_destroy(plans[i]);  // plans[0] may own the stream: last
    if (image) (void)hipFree(image);
}

real_t* VolumeDwt::sub_ptr(const SubBand& s) const {
    real_t* base = reinterpret_cast<real_t*>(pdwt_coeff_ptr(plans[s.level - 1], s.band));
    return base ? base + (long long)s.half * s.elems() : nullptr;
}

// A_l: the image for l = 0, else the depth-low half of band A of level l's plan
real_t* VolumeDwt::approx_ptr(int l) const { return l == 0 ? image : reinterpret_cast<real_t*>(pdwt_coeff_ptr(plans[l - 1], 0)); }

real_t* VolumeDwt::stack_ptr(int l) const { return reinterpret_cast<real_t*>(pdwt_image_ptr(plans[l - 1])); }

int VolumeDwt::copy(void* dst, const void* src, long long count, int kind) { return pdwt_copy(plans[0], dst, src, count, kind); }

int VolumeDwt::walk_steps(int level, bool inverse) const { return dwt3_depth_steps(nz[level - 1], hlen, inverse); }

int VolumeDwt::forward_levels() {
    for (int l = 1; l <= nlevels; l++) {
        pdwt_handle p = plans[l - 1];
        real_t* st = stack_ptr(l);
        const long long P = (long long)nr[l - 1] * nc[l - 1];
        const hipError_t e = launch_dwt3_depth_fwd(approx_ptr(l - 1), st, nz[l - 1], P, hlen, dec, seg_fwd[l - 1], stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "depth analysis of level %d failed: %s", l, hipGetErrorString(e));
        PDWT_TRY(pdwt_set_image(p, st, 1));  // written in place: nothing is copied
        PDWT_TRY(pdwt_forward(p));
    }
    return PDWT_OK;
}

int VolumeDwt::inverse_levels() {
    for (int l = nlevels; l >= 1; l--) {
        pdwt_handle p = plans[l - 1];
        // band A's depth-low half was written in place: by the level below, by the forward or by set_coeff
        PDWT_TRY(pdwt_set_coeff(p, reinterpret_cast<const real_t*>(pdwt_coeff_ptr(p, 0)), 0, 1));
        PDWT_TRY(pdwt_inverse(p));
        const long long P = (long long)nr[l - 1] * nc[l - 1];
        const hipError_t e = launch_dwt3_depth_inv(stack_ptr(l), approx_ptr(l - 1), nz[l - 1], P, hlen, rec, seg_inv[l - 1], stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "depth synthesis of level %d failed: %s", l, hipGetErrorString(e));
    }
    return PDWT_OK;
}

// every plan's table is [band][image]: the level's threshold everywhere but on the depth-low half of band A
int VolumeDwt::threshold(int op, const real_t* level_betas, real_t app_beta_or_nan, const char*) {
    // (plan_sweep_bands: pdwt_threshold_bands for every element-wise operator -- proj_linf and shrink come this way too)
    PDWT_TRY(mark_current(this));
    std::vector<real_t> table;
    for (int l = 1; l <= nlevels; l++) {
        const int half = nz[l], batch = 2 * half;
        table.assign((size_t)4 * batch, level_betas[l - 1]);
        const real_t low_a = l == nlevels ? app_beta_or_nan : kLeave;  // A_L, or an intermediate
        for (int i = 0; i < half; i++) table[i] = low_a;
        PDWT_TRY(plan_sweep_bands(plans[l - 1], op, table.data(), 0, "threshold_bands"));
    }
    return PDWT_OK;
}

int VolumeDwt::enter_sweep(const char*) { return mark_current(this); }

// c += alpha c_other over every level's whole coefficient region (launch_axpy, as pdwt_add_wavelet): the padding stays zero, and
// the intermediates A_1 .. A_{L-1} take part, which nothing can see -- the inverse overwrites A_{l-1} before it reads it, the
// forward writes it, and no getter or operator reaches it
int VolumeDwt::axpy(const pdwt_volume* other, real_t alpha) {
    const VolumeDwt* src = static_cast<const VolumeDwt*>(other);
    for (int l = 1; l <= nlevels; l++) {
        const pdwt_plan* d = plans[l - 1];
        const pdwt_plan* s = src->plans[l - 1];
        if (d->coeff_elems != s->coeff_elems) return VFAIL(PDWT_ERR_MISMATCH, "add_wavelet: level %d is laid out differently", l);
        HIP_TRY(launch_axpy(d->arena, s->arena, d->coeff_elems, alpha, stream));
    }
    return PDWT_OK;
}

int VolumeDwt::norms(double out[2]) {
    const int L = nlevels;
    std::vector<std::vector<double>> sums(L);  // [l - 1]: [band][image][2]
    for (int l = 1; l <= L; l++) {
        pdwt_handle p = plans[l - 1];
        double* d_stats = nullptr;
        PDWT_TRY(pdwt_band_stats_async(p, nullptr));
        PDWT_TRY(pdwt_adaptive_slots(p, &d_stats, nullptr, nullptr));
        sums[l - 1].resize((size_t)4 * 2 * nz[l] * 2);
        HIP_TRY(hipMemcpyAsync(sums[l - 1].data(), d_stats, sums[l - 1].size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    sum_norms(L, nz.data(), [&](int l, int b, int i) { return &sums[l - 1][((size_t)b * 2 * nz[l] + i) * 2]; }, out);
    return PDWT_OK;
}

int VolumeDwt::set_filters(int n, const real_t* dec_lo, const real_t* dec_hi, const real_t* rec_lo, const real_t* rec_hi) {
    // the level plans first: a plan that refuses leaves the volume's own bank as it was
    for (pdwt_handle p : plans) {
        PDWT_TRY(pdwt_set_filters_forward(p, nullptr, (unsigned)n, dec_lo, dec_hi, nullptr, nullptr));
        PDWT_TRY(pdwt_set_filters_inverse(p, rec_lo, rec_hi, nullptr, nullptr));
    }
    return pdwt_volume::set_filters(n, dec_lo, dec_hi, rec_lo, rec_hi);
}

// ---------------------------------------------------------------- the stationary volume
VolumeSwt::~VolumeSwt() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (block) (void)hipFree(block);
    if (group_ws) (void)hipFree(group_ws);
    if (spin_block) (void)hipFree(spin_block);
    if (h_table) (void)hipHostFree(h_table);
    if (staged) (void)hipEventDestroy(staged);
    if (own_stream && stream) (void)hipStreamDestroy(stream);
}

real_t* VolumeSwt::sub_ptr(const SubBand& s) const { return band[4 * (s.level - 1) + s.band] + (long long)s.half * s.elems(); }

real_t* VolumeSwt::approx_ptr(int l) const { return l == 0 ? image : band[4 * (l - 1)]; }

// as pdwt_copy does for a plan
int VolumeSwt::copy(void* dst, const void* src, long long count, int kind) {
    if (count == 0) return PDWT_OK;
    const hipMemcpyKind k = kind == 0 ? hipMemcpyDeviceToDevice : (kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)count * sizeof(real_t), k, stream));
    if (kind != 0) HIP_TRY(hipStreamSynchronize(stream));
    return PDWT_OK;
}

// the steps of one orbit walk at the level's dilation, the same in both directions
int VolumeSwt::walk_steps(int level, bool) const { return swt3_depth_steps(Nz, 1 << (level - 1)); }

Swt2DArgs VolumeSwt::level_args(int l, bool inverse) const {
    Swt2DArgs a;
    real_t* const* b = &band[4 * (l - 1)];
    a.in = inverse ? nullptr : stack;
    a.A = b[0], a.H = b[1], a.V = b[2], a.D = b[3];
    a.out = inverse ? stack : nullptr;
    a.Nr = Nr, a.Nc = Nc, a.f = 1 << (l - 1);
    a.bstride = (long long)Nr * Nc;
    a.hlen = hlen;
    a.soft_beta = 0;
    a.fb = inverse ? rec : dec;
    return a;
}

int VolumeSwt::forward_levels() {
    const long long P = (long long)Nr * Nc;
    const int B = 2 * Nz;
    for (int l = 1; l <= nlevels; l++) {
        hipError_t e = launch_swt3_depth_fwd(approx_ptr(l - 1), stack, Nz, P, 1 << (l - 1), hlen, dec, seg_fwd[l - 1], stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "depth analysis of level %d failed: %s", l, hipGetErrorString(e));
        const Swt2DArgs a = level_args(l, false);
        // the one-launch level first (plan.cpp: fwd_level_2d); hipErrorNotSupported is a decline
        e = swt2_fwd_stream_takes(a, B) ? try_launch_swt2_fwd_stream(a, B, stream) : hipErrorNotSupported;
        if (e == hipErrorNotSupported) e = launch_swt2_fwd(a, B, stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "2D analysis of level %d failed: %s", l, hipGetErrorString(e));
    }
    return PDWT_OK;
}

int VolumeSwt::inverse_levels() {
    const long long P = (long long)Nr * Nc;
    const int B = 2 * Nz;
    for (int l = nlevels; l >= 1; l--) {
        const Swt2DArgs a = level_args(l, true);
        hipError_t e = swt2_inv_stream_takes(a, B) ? try_launch_swt2_inv_stream(a, B, stream) : hipErrorNotSupported;
        if (e == hipErrorNotSupported) e = launch_swt2_inv(a, B, stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "2D synthesis of level %d failed: %s", l, hipGetErrorString(e));
        e = launch_swt3_depth_inv(stack, approx_ptr(l - 1), Nz, P, 1 << (l - 1), hlen, rec, seg_inv[l - 1], stream);
        if (e != hipSuccess) return VFAIL(PDWT_ERR_HIP, "depth synthesis of level %d failed: %s", l, hipGetErrorString(e));
    }
    return PDWT_OK;
}

// the sweeps see a level as 4 bands x 2 "images" of Nz P values; bands of 2^31 values and more are beyond their index math
int VolumeSwt::ops_check(const char* what) const {
    if ((long long)Nz * Nr * Nc >= (1LL << 31))
        return VFAIL(PDWT_ERR_UNSUPPORTED, "%s: sub-bands of %lld elements are beyond the operators' limit of 2^31 - 1", what, (long long)Nz * Nr * Nc);
    return PDWT_OK;
}

int VolumeSwt::enter_sweep(const char* what) { return ops_check(what); }

// the 4 L band arrays lie one behind the other, 256-B padded: one sweep (see VolumeDwt::axpy for the intermediates)
int VolumeSwt::axpy(const pdwt_volume* other, real_t alpha) {
    const VolumeSwt* src = static_cast<const VolumeSwt*>(other);
    const long long per = band[1] - band[0];
    HIP_TRY(launch_axpy(band[0], src->band[0], per * 4 * nlevels, alpha, stream));
    return PDWT_OK;
}

int VolumeSwt::threshold(int op, const real_t* level_betas, real_t app_beta_or_nan, const char* what) {
    PDWT_TRY(ops_check(what));
    const int L = nlevels;
    HIP_TRY(hipEventSynchronize(staged));  // the previous table has left the pinned buffer
    for (int l = 1; l <= L; l++) {
        for (int k = 0; k < 8; k++) h_table[8 * (l - 1) + k] = level_betas[l - 1];
        h_table[8 * (l - 1)] = l == L ? app_beta_or_nan : kLeave;  // aaa: A_L, or an intermediate
    }
    HIP_TRY(hipMemcpyAsync(table, h_table, (size_t)8 * L * sizeof(real_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(staged, stream));
    for (int l = 1; l <= L; l++)
        HIP_TRY(launch_threshold_bands(op, reinterpret_cast<real_t*>(block), bt[l - 1], table + 8 * (l - 1), stream));
    return PDWT_OK;
}

int VolumeSwt::norms(double out[2]) {
    PDWT_TRY(ops_check("norms"));
    const int L = nlevels;
    for (int l = 1; l <= L; l++)
        HIP_TRY(launch_band_stats(reinterpret_cast<const real_t*>(block), bt[l - 1], partial + (size_t)2 * pieces * (l - 1), stats + 16 * (l - 1), stream));
    std::vector<double> sums((size_t)16 * L);  // [level][band][half][2]
    HIP_TRY(hipMemcpyAsync(sums.data(), stats, sums.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const std::vector<int> one(L + 1, 1);  // a depth half is one "image"
    sum_norms(L, one.data(), [&](int l, int b, int i) { return &sums[(size_t)16 * (l - 1) + 2 * (2 * b + i)]; }, out);
    return PDWT_OK;
}

}  // namespace pdwt

namespace {

// the global soft / hard threshold of either volume
int threshold_entry(pdwt_volume_handle v, int op, real_t beta, int do_app, int normalize, const char* what) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "%s: cannot threshold coefficients, as they were modified by inverse()", what);
    DeviceGuard guard(v->device);
    std::vector<real_t> level_betas;
    const real_t a = level_thresholds(beta, v->nlevels, do_app, normalize, &level_betas);
    return v->threshold(op, level_betas.data(), a, what);
}

// proj_linf / shrink: one value for every detail sub-band, and for A_L when asked for, through the sweep of the thresholds
int uniform_entry(pdwt_volume_handle v, int op, real_t value, int do_app, const char* what) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "%s: cannot threshold coefficients, as they were modified by inverse()", what);
    DeviceGuard guard(v->device);
    const std::vector<real_t> per((size_t)v->nlevels, value);
    return v->threshold(op, per.data(), do_app ? value : kLeave, what);
}

int group_norm_entry(pdwt_volume_handle v, int do_app, double* d_out, double** d_slot) {
    if (v->state == PDWT_INVERSE) return VFAIL(PDWT_ERR_STATE, "group_norm: the coefficients were modified by inverse()");
    PDWT_TRY(v->enter_sweep("group_norm"));
    PDWT_TRY(ensure_group_ws(v));
    double* out = d_out ? d_out : v->group_ws;
    HIP_TRY(launch_vol_group_norm(v->groups, do_app ? 1 : 0, v->group_ws + 1, out, v->stream));
    if (d_slot) *d_slot = out;
    return PDWT_OK;
}

// what `later` is given from now on runs after what `earlier` holds now; the host does not wait
int order_after(hipStream_t later, hipStream_t earlier) {
    if (later == earlier) return PDWT_OK;
    hipEvent_t done = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    hipError_t e = hipEventRecord(done, earlier);
    if (e == hipSuccess) e = hipStreamWaitEvent(later, done, 0);
    (void)hipEventDestroy(done);  // (released once it has completed)
    HIP_TRY(e);
    return PDWT_OK;
}

// data into a sub-band or the image: nothing moves where the caller passes the destination itself
int copy_in(pdwt_volume_handle v, real_t* dst, const pdwt_real* src, long long count, int mem_is_on_device) {
    if (mem_is_on_device && src == dst) return PDWT_OK;
    PDWT_TRY(v->copy(dst, src, count, mem_is_on_device ? 0 : 1));
    if (mem_is_on_device) HIP_TRY(hipStreamSynchronize(v->stream));  // like pdwt_set_image: the source may be reused at once
    return PDWT_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pdwt_volume_layout(int Nz, int Nr, int Nc, const char* wname, int levels, int* nlevels, int* dims, int capacity) {
    const WaveletEntry* w = nullptr;
    PDWT_TRY(check_shape("pdwt_volume_layout", Nz, Nr, Nc, wname, kMaxDepthDwt, &w));
    const int L = clamp_levels(Nz, Nr, Nc, wname, w->hlen, levels, false);
    if (nlevels) *nlevels = L;
    int z = Nz, r = Nr, c = Nc;
    for (int l = 1; l <= L; l++) {
        z = div2(z), r = div2(r), c = div2(c);
        for (int k = 0; k < 7; k++) {
            const int num = 1 + 7 * (l - 1) + k;
            if (dims && num < capacity) dims[3 * num] = z, dims[3 * num + 1] = r, dims[3 * num + 2] = c;
        }
    }
    if (dims && capacity > 0) dims[0] = z, dims[1] = r, dims[2] = c;
    return 1 + 7 * L;
}

int pdwt_volume_create(const pdwt_real* img, int Nz, int Nr, int Nc, const char* wname, int levels, int mem_is_on_host,
                       int device_id, void* hip_stream, pdwt_volume_handle* out) {
    const char* what = "pdwt_volume_create";
    VolumeDwt* v = nullptr;
    PDWT_TRY(open_volume(what, Nz, Nr, Nc, wname, levels, kMaxDepthDwt, device_id, out, &v));
    DeviceGuard guard(device_id);
    auto bail = [&](int code) {
        delete v;
        return code;
    };
    const int L = v->nlevels;
    v->nz.assign(1, Nz), v->nr.assign(1, Nr), v->nc.assign(1, Nc);
    void* stream = hip_stream;
    for (int l = 1; l <= L; l++) {
        pdwt_handle p = nullptr;
        const int rc = pdwt_create_batched(nullptr, 2 * div2(v->nz[l - 1]), v->nr[l - 1], v->nc[l - 1], wname, 1, 0, 1, 0, 0, 2,
                                           device_id, stream, &p);
        if (rc != PDWT_OK) return bail(rc);
        v->plans.push_back(p);
        stream = pdwt_get_stream(p);  // level 1's private stream (or the caller's) serves every level
        v->nz.push_back(div2(v->nz[l - 1])), v->nr.push_back(div2(v->nr[l - 1])), v->nc.push_back(div2(v->nc[l - 1]));
    }
    v->stream = (hipStream_t)stream;
    build_ranges(v);
    build_groups(v);
    const size_t bytes = (size_t)Nz * Nr * Nc * sizeof(real_t);
    hipError_t e = hipMalloc((void**)&v->image, bytes);
    if (e != hipSuccess) {
        v->image = nullptr;
        VFAIL(PDWT_ERR_NOMEM, "%s: hipMalloc of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
        return bail(PDWT_ERR_NOMEM);
    }
    e = upload_image(v, img, mem_is_on_host);
    if (e != hipSuccess) {
        VFAIL(PDWT_ERR_HIP, "%s: image upload failed: %s", what, hipGetErrorString(e));
        return bail(PDWT_ERR_HIP);
    }
    // depth segments: fixed with the layout (every buffer is 256-B aligned, so the width depends on the plane size only); the
    // chooser aims at the workgroups the chip keeps resident of THAT kernel (2 per CU at 40 taps, 8 for short filters)
    for (int l = 1; l <= L; l++) {
        const long long P = (long long)v->nr[l - 1] * v->nc[l - 1];
        const int width = dwt3_depth_width(v->approx_ptr(l - 1), v->stack_ptr(l), P, v->hlen);
        v->width.push_back(width);
        v->seg_fwd.push_back(dwt3_depth_seg(v->nz[l - 1], P, v->hlen, width, false, dwt3_depth_slots(v->hlen, width, false)));
        v->seg_inv.push_back(dwt3_depth_seg(v->nz[l - 1], P, v->hlen, width, true, dwt3_depth_slots(v->hlen, width, true)));
    }
    v->seg_fwd_chosen = v->seg_fwd, v->seg_inv_chosen = v->seg_inv;
    *out = v;
    return PDWT_OK;
}

int pdwt_volume_create_swt(const pdwt_real* img, int Nz, int Nr, int Nc, const char* wname, int levels, int mem_is_on_host,
                           int device_id, void* hip_stream, pdwt_volume_handle* out) {
    const char* what = "pdwt_volume_create_swt";
    VolumeSwt* v = nullptr;
    PDWT_TRY(open_volume(what, Nz, Nr, Nc, wname, levels, kMaxDepthSwt, device_id, out, &v));
    DeviceGuard guard(device_id);
    auto bail = [&](int code) {
        delete v;
        return code;
    };
    const int L = v->nlevels;
    v->nz.assign(L + 1, Nz), v->nr.assign(L + 1, Nr), v->nc.assign(L + 1, Nc);
    if (hip_stream) {
        v->stream = (hipStream_t)hip_stream;
    } else {
        const hipError_t e = hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            v->stream = nullptr;
            VFAIL(PDWT_ERR_HIP, "%s: hipStreamCreate: %s", what, hipGetErrorString(e));
            return bail(PDWT_ERR_HIP);
        }
        v->own_stream = true;
    }
    const SwtLayout y = swt_layout(Nz, Nr, Nc, L, sizeof(real_t));
    hipError_t e = hipMalloc(&v->block, y.total);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        v->block = nullptr;
        VFAIL(PDWT_ERR_NOMEM, "%s: hipMalloc of %zu bytes failed: %s", what, y.total, hipGetErrorString(e));
        return bail(PDWT_ERR_NOMEM);
    }
    char* base = static_cast<char*>(v->block);
    v->image = reinterpret_cast<real_t*>(base + y.image);
    v->stack = reinterpret_cast<real_t*>(base + y.stack);
    for (int k = 0; k < 4 * L; k++) v->band.push_back(reinterpret_cast<real_t*>(base + y.bands + (size_t)k * y.band));
    v->stats = reinterpret_cast<double*>(base + y.stats);
    v->partial = reinterpret_cast<double*>(base + y.partial);
    v->table = reinterpret_cast<real_t*>(base + y.table);
    v->pieces = y.pieces;
    build_groups(v);
    const long long n = (long long)Nz * Nr * Nc;
    for (int l = 1; l <= L; l++) {
        BandTable t{};
        t.nbands = 4;
        t.batch = 2;
        t.chunk = y.chunk;
        for (int b = 0; b < 4; b++) {
            t.off[b] = (long long)((y.bands + (size_t)(4 * (l - 1) + b) * y.band) / sizeof(real_t));
            t.n[b] = n;
            t.blk[b] = b * (y.pieces / 4);
        }
        t.blk[4] = y.pieces;
        v->bt.push_back(t);
    }
    // everything behind the image starts as zeros: coefficients that were never computed read as 0, like a plan's arena
    e = hipMemsetAsync(base + y.stack, 0, y.total - y.stack, v->stream);
    if (e == hipSuccess) e = upload_image(v, img, mem_is_on_host);
    if (e == hipSuccess) e = hipHostMalloc((void**)&v->h_table, (size_t)8 * L * sizeof(real_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->staged, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        VFAIL(PDWT_ERR_HIP, "%s: image upload failed: %s", what, hipGetErrorString(e));
        return bail(PDWT_ERR_HIP);
    }
    // orbit segments: fixed with the layout (every buffer is 256-B aligned, so the widths depend on the plane size only)
    const long long P = (long long)Nr * Nc;
    for (int l = 1; l <= L; l++) {
        const int f = 1 << (l - 1);
        const int wf = swt3_depth_width(v->approx_ptr(l - 1), v->stack, P, v->hlen, false);
        const int wi = swt3_depth_width(v->stack, v->approx_ptr(l - 1), P, v->hlen, true);
        v->width.push_back(wf);
        v->width_inv.push_back(wi);
        v->seg_fwd.push_back(swt3_depth_seg(Nz, f, P, v->hlen, wf, swt3_depth_slots(v->hlen, wf, false)));
        v->seg_inv.push_back(swt3_depth_seg(Nz, f, P, v->hlen, wi, swt3_depth_slots(v->hlen, wi, true)));
    }
    v->seg_fwd_chosen = v->seg_fwd, v->seg_inv_chosen = v->seg_inv;
    *out = v;
    return PDWT_OK;
}

int pdwt_volume_is_swt(pdwt_volume_handle v) { return v ? v->do_swt : VFAIL(PDWT_ERR_ARG, "null volume handle"); }

int pdwt_volume_layout_swt(int Nz, int Nr, int Nc, const char* wname, int levels, int* nlevels, long long* device_bytes, int sizeof_real) {
    const WaveletEntry* w = nullptr;
    PDWT_TRY(check_shape("pdwt_volume_layout_swt", Nz, Nr, Nc, wname, kMaxDepthSwt, &w));
    if (sizeof_real != 0 && sizeof_real != 4 && sizeof_real != 8)
        return VFAIL(PDWT_ERR_ARG, "pdwt_volume_layout_swt: sizeof_real must be 4, 8 or 0 (this library's), got %d", sizeof_real);
    const int L = clamp_levels(Nz, Nr, Nc, wname, w->hlen, levels, false);
    if (nlevels) *nlevels = L;
    if (device_bytes) *device_bytes = (long long)swt_layout(Nz, Nr, Nc, L, sizeof_real ? (size_t)sizeof_real : sizeof(real_t)).total;
    return 1 + 7 * L;
}

int pdwt_volume_destroy(pdwt_volume_handle v) {
    if (!v) return PDWT_OK;
    DeviceGuard guard(v->device);
    delete v;
    return PDWT_OK;
}

int pdwt_volume_forward(pdwt_volume_handle v) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    DeviceGuard guard(v->device);
    int rc = PDWT_OK;
    if (v->do_cycle_spinning) {  // wt.cu:242-246, on three axes (plan.cpp: pdwt_forward)
        const int n[3] = {v->Nz, v->Nr, v->Nc};
        int d[3];
        for (int a = 0; a < 3; a++) d[a] = (int)(spin_draw(v) % (unsigned long long)n[a]);
        rc = shift_image(v, d[0], d[1], d[2]);
        for (int a = 0; a < 3 && rc == PDWT_OK; a++) v->shift[a] = vol_shift_reduce((long long)v->shift[a] + d[a], n[a]);
    }
    if (rc == PDWT_OK) rc = v->forward_levels();
    v->state = rc == PDWT_OK ? PDWT_FORWARD : PDWT_FORWARD_ERROR;
    return rc;
}

int pdwt_volume_inverse(pdwt_volume_handle v) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "W.inverse() has already been run. Inverse is available in W.get_image()");
    if (v->state == PDWT_FORWARD_ERROR || v->state == PDWT_THRESHOLD_ERROR || v->state == PDWT_CREATION_ERROR)
        return VFAIL(PDWT_ERR_STATE, "inverse transform not computed, as there was an error in a previous stage");
    DeviceGuard guard(v->device);
    int rc = v->inverse_levels();
    if (rc == PDWT_OK && v->do_cycle_spinning) {  // wt.cu:303
        rc = shift_image(v, -v->shift[0], -v->shift[1], -v->shift[2]);
        if (rc == PDWT_OK) v->shift[0] = v->shift[1] = v->shift[2] = 0;
    }
    v->state = rc == PDWT_OK ? PDWT_INVERSE : PDWT_INVERSE_ERROR;
    return rc;
}

int pdwt_volume_get_info(pdwt_volume_handle v, int* Nz, int* Nr, int* Nc, int* nlevels, int* hlen, int* state) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (Nz) *Nz = v->Nz;
    if (Nr) *Nr = v->Nr;
    if (Nc) *Nc = v->Nc;
    if (nlevels) *nlevels = v->nlevels;
    if (hlen) *hlen = v->hlen;
    if (state) *state = v->state;
    return PDWT_OK;
}

long long pdwt_volume_get_image(pdwt_volume_handle v, pdwt_real* dst) {
    if (!v || !dst) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_get_image: null argument");
    DeviceGuard guard(v->device);
    const long long n = (long long)v->Nz * v->Nr * v->Nc;
    PDWT_TRY(v->copy(dst, v->image, n, 2));
    return n;
}

int pdwt_volume_set_image(pdwt_volume_handle v, const pdwt_real* src, int mem_is_on_device) {
    if (!v || !src) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_image: null argument");
    DeviceGuard guard(v->device);
    PDWT_TRY(copy_in(v, v->image, src, (long long)v->Nz * v->Nr * v->Nc, mem_is_on_device));
    v->state = PDWT_INIT;
    v->shift[0] = v->shift[1] = v->shift[2] = 0;  // (a cycle-spinning volume: the new image is not shifted)
    return PDWT_OK;
}

long long pdwt_volume_coeff_count(pdwt_volume_handle v, int num, int* depth, int* rows, int* cols) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    SubBand s;
    if (!locate(v, num, &s)) return VFAIL(PDWT_ERR_ARG, "coefficient index %d out of range", num);
    if (depth) *depth = s.depth;
    if (rows) *rows = s.rows;
    if (cols) *cols = s.cols;
    return s.elems();
}

long long pdwt_volume_get_coeff(pdwt_volume_handle v, pdwt_real* dst, int num) {
    if (!v || !dst) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_get_coeff: null argument");
    SubBand s;
    if (!locate(v, num, &s)) return VFAIL(PDWT_ERR_ARG, "coefficient index %d out of range", num);
    if (v->state == PDWT_INVERSE) {  // 0 values, not an error code: pdwt_get_coeff (wt.cu:473-477)
        VFAIL(PDWT_ERR_STATE, "get_coeff(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    DeviceGuard guard(v->device);
    PDWT_TRY(v->copy(dst, v->sub_ptr(s), s.elems(), 2));
    return s.elems();
}

int pdwt_volume_set_coeff(pdwt_volume_handle v, const pdwt_real* src, int num, int mem_is_on_device) {
    if (!v || !src) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_coeff: null argument");
    SubBand s;
    if (!locate(v, num, &s)) return VFAIL(PDWT_ERR_ARG, "coefficient index %d out of range", num);
    DeviceGuard guard(v->device);
    PDWT_TRY(copy_in(v, v->sub_ptr(s), src, s.elems(), mem_is_on_device));
    // as pdwt_set_coeff: once the approximation has been supplied again the coefficients are current
    if (num == 0 && v->state == PDWT_INVERSE) v->state = PDWT_FORWARD;
    return PDWT_OK;
}

intptr_t pdwt_volume_image_ptr(pdwt_volume_handle v) { return v ? (intptr_t)v->image : 0; }

intptr_t pdwt_volume_coeff_ptr(pdwt_volume_handle v, int num) {
    SubBand s;
    if (!v || !locate(v, num, &s)) return 0;
    DeviceGuard guard(v->device);
    return (intptr_t)v->sub_ptr(s);
}

int pdwt_volume_soft_threshold(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs, int normalize) {
    return threshold_entry(v, EW_SOFT, beta, do_thresh_appcoeffs, normalize, "soft_threshold");
}

int pdwt_volume_hard_threshold(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs, int normalize) {
    return threshold_entry(v, EW_HARD, beta, do_thresh_appcoeffs, normalize, "hard_threshold");
}

int pdwt_volume_group_soft_threshold(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs, int normalize) {
    const char* what = "group_soft_threshold";
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "%s: cannot threshold coefficients, as they were modified by inverse()", what);
    DeviceGuard guard(v->device);
    PDWT_TRY(v->enter_sweep(what));
    // the group of level L takes beta_L with or without A_L: the approximation has no threshold of its own here
    std::vector<real_t> level_betas;
    (void)level_thresholds(beta, v->nlevels, 0, normalize, &level_betas);
    VolGroupBetas b{};
    for (int l = 0; l < v->nlevels; l++) b.b[l] = level_betas[l];
    HIP_TRY(launch_vol_group_soft(v->groups, b, do_thresh_appcoeffs ? 1 : 0, v->stream));
    return PDWT_OK;
}

int pdwt_volume_proj_linf(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs) {
    return uniform_entry(v, EW_LINF, beta, do_thresh_appcoeffs, "proj_linf");
}

int pdwt_volume_shrink(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs) {
    const real_t factor = 1.0f / (1.0f + beta);  // formed once, in real_t (pdwt_shrink, plan.cpp)
    return uniform_entry(v, EW_SCALE, factor, do_thresh_appcoeffs, "shrink");
}

int pdwt_volume_add_wavelet(pdwt_volume_handle dst, pdwt_volume_handle src, pdwt_real alpha) {
    if (!dst || !src) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (dst->nlevels != src->nlevels || strcasecmp(dst->wname, src->wname))
        return VFAIL(PDWT_ERR_MISMATCH, "add_wavelet(): right operand is not the same transform (wname, level)");
    if (dst->Nz != src->Nz || dst->Nr != src->Nr || dst->Nc != src->Nc)
        return VFAIL(PDWT_ERR_MISMATCH, "add_wavelet(): operands do not have the same geometry");
    if (dst->do_swt != src->do_swt) return VFAIL(PDWT_ERR_MISMATCH, "add_wavelet(): operands should both use SWT or DWT");
    if (dst->device != src->device) return VFAIL(PDWT_ERR_MISMATCH, "add_wavelet(): operands live on different devices");
    if (dst->state == PDWT_INVERSE || src->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "add_wavelet(): this operation makes no sense when wavelet has just been inverted");
    DeviceGuard guard(dst->device);
    PDWT_TRY(dst->enter_sweep("add_wavelet"));
    if (src != dst) PDWT_TRY(src->enter_sweep("add_wavelet"));
    // after what is queued on the source's stream, without stopping the host ...
    PDWT_TRY(order_after(dst->stream, src->stream));
    PDWT_TRY(dst->axpy(src, alpha));
    // ... and whatever the source's stream is given next waits until the sum has read the source: the caller's next call on
    // `src` (a threshold, a forward, set_coeff) would otherwise overwrite coefficients the sum is still reading
    return order_after(src->stream, dst->stream);
}

int pdwt_volume_group_norm_async(pdwt_volume_handle v, int do_thresh_appcoeffs, double* d_out, double** d_slot) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    DeviceGuard guard(v->device);
    return group_norm_entry(v, do_thresh_appcoeffs, d_out, d_slot);
}

int pdwt_volume_group_norm(pdwt_volume_handle v, int do_thresh_appcoeffs, double* out) {
    if (!v || !out) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_group_norm: null argument");
    DeviceGuard guard(v->device);
    PDWT_TRY(group_norm_entry(v, do_thresh_appcoeffs, nullptr, nullptr));
    HIP_TRY(hipMemcpyAsync(out, v->group_ws, sizeof(double), hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return PDWT_OK;
}

int pdwt_volume_norms(pdwt_volume_handle v, double out[2]) {
    if (!v || !out) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_norms: null argument");
    if (v->state == PDWT_INVERSE) return VFAIL(PDWT_ERR_STATE, "norms: the coefficients were modified by inverse()");
    DeviceGuard guard(v->device);
    return v->norms(out);
}

// ---------------------------------------------------------------- the adaptive and K-term operators on ONE (decimated) volume
int pdwt_volume_band_stats_async(pdwt_volume_handle h, double* d_out) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_band_stats_async", &v));
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "band_stats", false));
    return band_stats_impl(v, d_out);
}

int pdwt_volume_norms_async(pdwt_volume_handle h, double* d_out2) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_norms_async", &v));
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "norms", false));
    PDWT_TRY(band_stats_impl(v, nullptr));
    HIP_TRY(launch_vol_norms(v->ops->stats, num_bands(v), d_out2 ? d_out2 : v->ops->norms, v->stream));
    return PDWT_OK;
}

int pdwt_volume_estimate_sigma_async(pdwt_volume_handle h, int skip_zeros, double* d_out) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_estimate_sigma_async", &v));
    DeviceGuard guard(v->device);
    PDWT_TRY(noise_check(v, "estimate_sigma"));
    PDWT_TRY(enter_ops(v, "estimate_sigma", false));
    return estimate_sigma_impl(v, skip_zeros, d_out);
}

int pdwt_volume_threshold_bands(pdwt_volume_handle h, int op, const pdwt_real* table, int table_on_device) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_threshold_bands", &v));
    if (!table) return VFAIL(PDWT_ERR_ARG, "threshold_bands: null table");
    if (op != EW_SOFT && op != EW_HARD) return VFAIL(PDWT_ERR_ARG, "threshold_bands: op must be 0 (soft) or 1 (hard)");
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "threshold_bands", true));
    if (table_on_device) {
        HIP_TRY(launch_vol_expand(v->ops->levels, table, v->stream));
        return sweep_levels(v, op);
    }
    // a host table is expanded here and goes through every plan's own staging buffer
    std::vector<real_t> per;
    for (int l = 1; l <= v->nlevels; l++) {
        const int half = v->nz[l], batch = 2 * half;
        per.resize((size_t)4 * batch);
        for (int b = 0; b < 4; b++)
            for (int i = 0; i < batch; i++) {
                const int num = vol_num_of(l, v->nlevels, b, i, half);
                per[(size_t)b * batch + i] = num < 0 ? kLeave : table[num];
            }
        PDWT_TRY(pdwt_threshold_bands(v->plans[l - 1], op, per.data(), 0));
    }
    return PDWT_OK;
}

int pdwt_volume_denoise_async(pdwt_volume_handle h, int method, int op, const double* sigma, int skip_zeros) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_denoise_async", &v));
    if (method != PDWT_DENOISE_BAYES && method != PDWT_DENOISE_VISU) return VFAIL(PDWT_ERR_ARG, "denoise: unknown method %d", method);
    if (op != EW_SOFT && op != EW_HARD) return VFAIL(PDWT_ERR_ARG, "denoise: op must be 0 (soft) or 1 (hard)");
    if (!sigma) PDWT_TRY(noise_check(v, "denoise"));
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "denoise", true));
    if (sigma) PDWT_TRY(stage_upload(v, v->ops->sigma, sigma, sizeof(double)));
    return denoise_sweep(v, method, op, !sigma, skip_zeros);
}

int pdwt_volume_adaptive_slots(pdwt_volume_handle h, double** d_stats, double** d_sigma, pdwt_real** d_table) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_adaptive_slots", &v));
    DeviceGuard guard(v->device);
    PDWT_TRY(ensure_ops(v));
    if (d_stats) *d_stats = v->ops->stats;
    if (d_sigma) *d_sigma = v->ops->sigma;
    if (d_table) *d_table = v->ops->table;
    return PDWT_OK;
}

int pdwt_volume_select_magnitude_async(pdwt_volume_handle h, long long k, int do_thresh_appcoeffs, pdwt_real* d_threshold,
                                       unsigned long long* d_kept) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_select_magnitude_async", &v));
    PDWT_TRY(sparsify_check(v, "select_magnitude", k, do_thresh_appcoeffs));
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "select_magnitude", false));
    return select_magnitude_impl(v, k, do_thresh_appcoeffs, d_threshold, d_kept);
}

int pdwt_volume_keep_largest_async(pdwt_volume_handle h, long long k, int do_thresh_appcoeffs) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_keep_largest_async", &v));
    PDWT_TRY(sparsify_check(v, "keep_largest", k, do_thresh_appcoeffs));
    DeviceGuard guard(v->device);
    PDWT_TRY(enter_ops(v, "keep_largest", true));
    PDWT_TRY(select_magnitude_impl(v, k, do_thresh_appcoeffs, nullptr, nullptr));
    HIP_TRY(launch_vol_keep(v->rt_keep, do_thresh_appcoeffs ? 1 : 0, v->ops->sp_key, v->stream));
    return PDWT_OK;
}

int pdwt_volume_sparsify_slots(pdwt_volume_handle h, pdwt_real** d_threshold, unsigned long long** d_kept) {
    VolumeDwt* v = nullptr;
    PDWT_TRY(as_dwt(h, "pdwt_volume_sparsify_slots", &v));
    DeviceGuard guard(v->device);
    PDWT_TRY(ensure_ops(v));
    if (d_threshold) *d_threshold = v->ops->sp_threshold;
    if (d_kept) *d_kept = v->ops->sp_kept;
    return PDWT_OK;
}

// ---------------------------------------------------------------- circular shifts and cycle spinning
int pdwt_volume_circshift(pdwt_volume_handle v, int sz, int sr, int sc) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (!image_current(v)) return VFAIL(PDWT_ERR_STATE, "circshift: the image is not current (forward() has been run; call inverse() or set_image())");
    DeviceGuard guard(v->device);
    PDWT_TRY(shift_image(v, sz, sr, sc));
    v->state = PDWT_INIT;
    return PDWT_OK;
}

int pdwt_volume_set_cycle_spinning(pdwt_volume_handle v, int on, unsigned long long seed) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (on && v->do_swt)  // as pdwt_create refuses the combination for a 2D plan
        return VFAIL(PDWT_ERR_UNSUPPORTED, "cycle spinning is not built for stationary volumes (do_swt): the transform is translation invariant already");
    if (!on && v->do_cycle_spinning && (v->shift[0] || v->shift[1] || v->shift[2]))
        return VFAIL(PDWT_ERR_STATE, "set_cycle_spinning: the image is still shifted; run inverse() or set_image() first");
    v->do_cycle_spinning = on ? 1 : 0;
    v->rng = seed;
    return PDWT_OK;
}

int pdwt_volume_current_shift(pdwt_volume_handle v, int shift[3]) {
    if (!v || !shift) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_current_shift: null argument");
    for (int a = 0; a < 3; a++) shift[a] = v->shift[a];
    return PDWT_OK;
}

int pdwt_volume_spin_footprint(int Nz, int Nr, int Nc, size_t real_bytes, size_t* extra_bytes) {
    if (Nz < 1 || Nr < 1 || Nc < 1 || !extra_bytes) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_spin_footprint: bad arguments");
    if (real_bytes != 0 && real_bytes != 4 && real_bytes != 8)
        return VFAIL(PDWT_ERR_ARG, "pdwt_volume_spin_footprint: real_bytes must be 4, 8 or 0 (this library's), got %zu", real_bytes);
    *extra_bytes = 2 * spin_volume_bytes(Nz, Nr, Nc, real_bytes ? real_bytes : sizeof(real_t));
    return PDWT_OK;
}

int pdwt_volume_cycle_spin_async(pdwt_volume_handle h, int nshifts, const int* shifts, int op, double beta, int do_app, int normalize,
                                 int method, const double* sigma, int skip_zeros) {
    const char* what = "cycle_spin";
    VolumeDwt* v = nullptr;
    if (!h) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (h->do_swt)
        return VFAIL(PDWT_ERR_UNSUPPORTED, "%s: not built for stationary volumes (do_swt): the transform is translation invariant already", what);
    v = static_cast<VolumeDwt*>(h);
    if (nshifts < 1 || !shifts) return VFAIL(PDWT_ERR_ARG, "%s: at least one shift is needed", what);
    if (op != EW_SOFT && op != EW_HARD) return VFAIL(PDWT_ERR_ARG, "%s: op must be 0 (soft) or 1 (hard)", what);
    const bool adaptive = method != PDWT_SPIN_GLOBAL;
    if (adaptive && method != PDWT_DENOISE_BAYES && method != PDWT_DENOISE_VISU) return VFAIL(PDWT_ERR_ARG, "%s: unknown method %d", what, method);
    if (!image_current(v)) return VFAIL(PDWT_ERR_STATE, "%s: the image is not current (forward() has been run; call inverse() or set_image())", what);
    if (v->do_cycle_spinning) return VFAIL(PDWT_ERR_STATE, "%s: the volume draws a shift of its own per forward (set_cycle_spinning); the two would compose", what);
    if (adaptive && !sigma) PDWT_TRY(noise_check(v, what));
    DeviceGuard guard(v->device);
    PDWT_TRY(ensure_spin(v));
    if (adaptive) {
        PDWT_TRY(ensure_ops(v));
        if (sigma) PDWT_TRY(stage_upload(v, v->ops->sigma, sigma, sizeof(double)));  // once: nothing below writes the slot
    }
    std::vector<real_t> level_betas;
    const real_t app = level_thresholds((real_t)beta, v->nlevels, do_app, normalize, &level_betas);
    const long long n = (long long)v->Nz * v->Nr * v->Nc;
    const real_t w = (real_t)(1.0 / nshifts);
    int rc = v->copy(v->spin_src, v->image, n, 0);
    for (int s = 0; s < nshifts && rc == PDWT_OK; s++) {
        const int* d = shifts + 3 * s;
        hipError_t e = launch_vol_circshift(v->spin_src, v->image, v->Nz, v->Nr, v->Nc, d[0], d[1], d[2], v->stream);
        if (e != hipSuccess) rc = VFAIL(PDWT_ERR_HIP, "%s: shift %d failed: %s", what, s, hipGetErrorString(e));
        if (rc == PDWT_OK) rc = v->forward_levels();
        if (rc == PDWT_OK) {
            if (adaptive) {
                rc = mark_current(v);
                if (rc == PDWT_OK) rc = denoise_sweep(v, method, op, !sigma, skip_zeros);
            } else {
                rc = v->threshold(op, level_betas.data(), app, what);
            }
        }
        if (rc == PDWT_OK) rc = v->inverse_levels();
        if (rc == PDWT_OK) {
            e = launch_vol_unshift_acc(v->image, v->spin_acc, v->Nz, v->Nr, v->Nc, d[0], d[1], d[2], w, s == 0, v->stream);
            if (e != hipSuccess) rc = VFAIL(PDWT_ERR_HIP, "%s: accumulation of shift %d failed: %s", what, s, hipGetErrorString(e));
        }
    }
    if (rc == PDWT_OK) rc = v->copy(v->image, v->spin_acc, n, 0);
    v->state = rc == PDWT_OK ? PDWT_INVERSE : PDWT_INVERSE_ERROR;
    return rc;
}

int pdwt_volume_read(pdwt_volume_handle v, void* dst, const void* d_src, long long bytes) {
    if (!v || !dst || !d_src || bytes < 0) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_read: bad arguments");
    DeviceGuard guard(v->device);
    HIP_TRY(hipMemcpyAsync(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return PDWT_OK;
}

int pdwt_volume_synchronize(pdwt_volume_handle v) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    DeviceGuard guard(v->device);
    HIP_TRY(hipStreamSynchronize(v->stream));
    return PDWT_OK;
}

void* pdwt_volume_stream(pdwt_volume_handle v) { return v ? (void*)v->stream : nullptr; }

int pdwt_volume_depth_schedule(pdwt_volume_handle v, int level, int* width, int* seg_fwd, int* seg_inv) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (level < 1 || level > v->nlevels) return VFAIL(PDWT_ERR_ARG, "level %d out of range (1 .. %d)", level, v->nlevels);
    if (width) *width = v->width[level - 1];
    if (seg_fwd) *seg_fwd = v->seg_fwd[level - 1];
    if (seg_inv) *seg_inv = v->seg_inv[level - 1];
    return PDWT_OK;
}

// ---------------------------------------------------------------- test hooks (include/pypwt_amd_bench.h)
int pdwt_volume_set_filters(pdwt_volume_handle v, int hlen, const pdwt_real* dec_lo, const pdwt_real* dec_hi, const pdwt_real* rec_lo,
                            const pdwt_real* rec_hi) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (!dec_lo || !dec_hi || !rec_lo || !rec_hi) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_filters: null filter");
    if (hlen != v->hlen)
        return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_filters: %d taps, the volume was created with %d (the schedule is not rebuilt)", hlen, v->hlen);
    DeviceGuard guard(v->device);
    return v->set_filters(hlen, dec_lo, dec_hi, rec_lo, rec_hi);
}

int pdwt_volume_set_depth_segments(pdwt_volume_handle v, int level, int seg_fwd, int seg_inv) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (level < 1 || level > v->nlevels) return VFAIL(PDWT_ERR_ARG, "level %d out of range (1 .. %d)", level, v->nlevels);
    const int steps_fwd = v->walk_steps(level, false), steps_inv = v->walk_steps(level, true);
    if (seg_fwd < 0 || seg_fwd > steps_fwd || seg_inv < 0 || seg_inv > steps_inv)
        return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_depth_segments: (%d, %d) steps per segment, level %d walks (%d, %d) steps", seg_fwd, seg_inv,
                     level, steps_fwd, steps_inv);
    v->seg_fwd[level - 1] = seg_fwd ? seg_fwd : v->seg_fwd_chosen[level - 1];
    v->seg_inv[level - 1] = seg_inv ? seg_inv : v->seg_inv_chosen[level - 1];
    return PDWT_OK;
}

int pdwt_volume_depth_width(pdwt_volume_handle v, int level, int inverse) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (level < 1 || level > v->nlevels) return VFAIL(PDWT_ERR_ARG, "level %d out of range (1 .. %d)", level, v->nlevels);
    return v->depth_width(level, inverse != 0);
}

}  // extern "C"
#pragma GCC visibility pop
