// volume.cpp -- the pdwt_volume_* block of the C ABI (include/pypwt_amd.h): the 3D DWT of a volume as depth passes
// (launch_dwt3.hip) around one-level batched 2D plans (volume.hpp has the layout).  The 2D side goes through the plans' own
// entry points -- pdwt_create_batched, pdwt_forward / pdwt_inverse, pdwt_threshold_bands, pdwt_band_stats_async --, so nothing
// a 1D or 2D plan does is restated here.
#include "volume.hpp"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "launch.hpp"
#include "wavelet_table.hpp"

using namespace pdwt;

namespace {

#define VFAIL(code, ...) set_last_error((code), __VA_ARGS__)

#define HIP_TRY(expr)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                    \
            return VFAIL(PDWT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define PDWT_TRY(expr)                \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_ != PDWT_OK) return rc_; \
    } while (0)

int div2(int n) { return (n + (n & 1)) / 2; }

int ilog2(int i) {  // pdwt/src/utils.cu:14-20
    int l = 0;
    while (i > 1) {
        i >>= 1;
        ++l;
    }
    return l;
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        else if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// the seven detail sub-bands of a level in pywt.wavedecn's sorted key order, axes (z, y, x): depth half (0 low, 1 high) and
// band of the level's 2D plan (0 A, 1 H, 2 V, 3 D)
const struct { const char* key; int half, band; } kSub[7] = {
    {"aad", 0, 2}, {"ada", 0, 1}, {"add", 0, 3}, {"daa", 1, 0}, {"dad", 1, 2}, {"dda", 1, 1}, {"ddd", 1, 3}};

// argument checks shared by create and layout; no HIP call
int check_shape(const char* what, int Nz, int Nr, int Nc, const char* wname, const WaveletEntry** w) {
    if (Nz < 2 || Nr < 2 || Nc < 2) return VFAIL(PDWT_ERR_ARG, "%s: every axis needs at least 2 samples, got (%d, %d, %d)", what, Nz, Nr, Nc);
    // the per-band operators of a batched plan take at most 65535 images, and a level's plan holds 2 div2(Nz) of them
    if (Nz > 65534) return VFAIL(PDWT_ERR_ARG, "%s: depth %d is beyond the limit of 65534 slices", what, Nz);
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

int num_bands(const pdwt_volume* v) { return 1 + 7 * v->nlevels; }

struct SubBand {
    int level, half, band;  // level 1 .. L, depth half, band of that level's plan
    int depth, rows, cols;
};

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

long long elems(const SubBand& s) { return (long long)s.depth * s.rows * s.cols; }

real_t* sub_ptr(const pdwt_volume* v, const SubBand& s) {
    real_t* base = reinterpret_cast<real_t*>(pdwt_coeff_ptr(v->plans[s.level - 1], s.band));
    return base ? base + (long long)s.half * elems(s) : nullptr;
}

// A_l: the image for l = 0, else the depth-low half of band A of level l's plan
real_t* approx_ptr(const pdwt_volume* v, int l) {
    return l == 0 ? v->image : reinterpret_cast<real_t*>(pdwt_coeff_ptr(v->plans[l - 1], 0));
}

real_t* stack_ptr(const pdwt_volume* v, int l) { return reinterpret_cast<real_t*>(pdwt_image_ptr(v->plans[l - 1])); }

// every level's plan is told that its coefficients are current: they were written in place (pypwt_amd/tiled.py:431-437)
int mark_current(pdwt_volume* v) {
    for (pdwt_handle p : v->plans) PDWT_TRY(pdwt_set_coeff(p, reinterpret_cast<const real_t*>(pdwt_coeff_ptr(p, 0)), 0, 1));
    return PDWT_OK;
}

real_t app_beta(real_t beta, int levels, int normalize) {  // plan.cpp: app_beta (pdwt/src/common.cu:229-236)
    if (normalize > 0) {
        const int n2 = levels / 2;
        beta /= (real_t)(1 << n2);
        if (n2 * 2 != levels) beta = (real_t)(beta / 1.4142135623730951);
    }
    return beta;
}

int threshold_impl(pdwt_volume* v, int op, real_t beta, int do_app, int normalize, const char* what) {
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "%s: cannot threshold coefficients, as they were modified by inverse()", what);
    DeviceGuard guard(v->device);
    PDWT_TRY(mark_current(v));
    const int L = v->nlevels;
    const real_t leave = std::numeric_limits<real_t>::quiet_NaN();  // pdwt_threshold_bands: a NaN entry leaves that (band, image) alone
    std::vector<real_t> table;
    real_t b = beta;
    for (int l = 1; l <= L; l++) {
        if (normalize > 0) b = (real_t)(b / 1.4142135623730951);  // plan.cpp: threshold_sweep (common.cu:244)
        const int half = v->nz[l], batch = 2 * half;
        table.assign((size_t)4 * batch, b);
        const real_t low_a = (l == L && do_app) ? app_beta(beta, L, normalize) : leave;
        for (int i = 0; i < half; i++) table[i] = low_a;
        PDWT_TRY(pdwt_threshold_bands(v->plans[l - 1], op, table.data(), 0));
    }
    return PDWT_OK;
}

void destroy(pdwt_volume* v) {
    DeviceGuard guard(v->device);
    if (!v->plans.empty()) (void)hipStreamSynchronize(v->stream);
    for (size_t i = v->plans.size(); i-- > 0;) pdwt_destroy(v->plans[i]);  // plans[0] may own the stream: last
    if (v->image) (void)hipFree(v->image);
    delete v;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int pdwt_volume_layout(int Nz, int Nr, int Nc, const char* wname, int levels, int* nlevels, int* dims, int capacity) {
    const WaveletEntry* w = nullptr;
    PDWT_TRY(check_shape("pdwt_volume_layout", Nz, Nr, Nc, wname, &w));
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
    if (!out) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_create: out is null");
    *out = nullptr;
    const WaveletEntry* w = nullptr;
    PDWT_TRY(check_shape("pdwt_volume_create", Nz, Nr, Nc, wname, &w));

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return VFAIL(PDWT_ERR_HIP, "no HIP device available (this library has no CPU path)");
    if (device_id < 0) HIP_TRY(hipGetDevice(&device_id));
    if (device_id >= ndev) return VFAIL(PDWT_ERR_ARG, "device %d out of range (%d devices)", device_id, ndev);

    pdwt_volume* v = new pdwt_volume();
    v->device = device_id;
    v->Nz = Nz, v->Nr = Nr, v->Nc = Nc;
    v->hlen = w->hlen;
    v->nlevels = clamp_levels(Nz, Nr, Nc, wname, w->hlen, levels, true);
    snprintf(v->wname, sizeof(v->wname), "%s", wname);
    for (int i = 0; i < kMaxTaps; i++) {
        const bool in = i < w->hlen;
        v->dec.lo[i] = in ? (real_t)w->dec_lo[i] : 0, v->dec.hi[i] = in ? (real_t)w->dec_hi[i] : 0;
        v->rec.lo[i] = in ? (real_t)w->rec_lo[i] : 0, v->rec.hi[i] = in ? (real_t)w->rec_hi[i] : 0;
    }
    DeviceGuard guard(device_id);
    auto bail = [&](int code) {
        destroy(v);
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
    const size_t bytes = (size_t)Nz * Nr * Nc * sizeof(real_t);
    hipError_t e = hipMalloc((void**)&v->image, bytes);
    if (e != hipSuccess) {
        v->image = nullptr;
        VFAIL(PDWT_ERR_NOMEM, "pdwt_volume_create: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return bail(PDWT_ERR_NOMEM);
    }
    e = img ? hipMemcpyAsync(v->image, img, bytes, mem_is_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, v->stream)
            : hipMemsetAsync(v->image, 0, bytes, v->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(v->stream);
    if (e != hipSuccess) {
        VFAIL(PDWT_ERR_HIP, "pdwt_volume_create: image upload failed: %s", hipGetErrorString(e));
        return bail(PDWT_ERR_HIP);
    }
    // depth segments: fixed with the layout (every buffer is 256-B aligned, so the width depends on the plane size only); the
    // chooser aims at the workgroups the chip keeps resident of THAT kernel (2 per CU at 40 taps, 8 for short filters)
    for (int l = 1; l <= L; l++) {
        const long long P = (long long)v->nr[l - 1] * v->nc[l - 1];
        const int width = dwt3_depth_width(approx_ptr(v, l - 1), stack_ptr(v, l), P, v->hlen);
        v->width.push_back(width);
        v->seg_fwd.push_back(dwt3_depth_seg(v->nz[l - 1], P, v->hlen, width, false, dwt3_depth_slots(v->hlen, width, false)));
        v->seg_inv.push_back(dwt3_depth_seg(v->nz[l - 1], P, v->hlen, width, true, dwt3_depth_slots(v->hlen, width, true)));
    }
    *out = v;
    return PDWT_OK;
}

int pdwt_volume_destroy(pdwt_volume_handle v) {
    if (!v) return PDWT_OK;
    destroy(v);
    return PDWT_OK;
}

int pdwt_volume_forward(pdwt_volume_handle v) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    DeviceGuard guard(v->device);
    for (int l = 1; l <= v->nlevels; l++) {
        pdwt_handle p = v->plans[l - 1];
        real_t* stack = stack_ptr(v, l);
        const long long P = (long long)v->nr[l - 1] * v->nc[l - 1];
        const hipError_t e = launch_dwt3_depth_fwd(approx_ptr(v, l - 1), stack, v->nz[l - 1], P, v->hlen, v->dec, v->seg_fwd[l - 1], v->stream);
        int rc = e == hipSuccess ? PDWT_OK : VFAIL(PDWT_ERR_HIP, "depth analysis of level %d failed: %s", l, hipGetErrorString(e));
        if (rc == PDWT_OK) rc = pdwt_set_image(p, stack, 1);  // written in place: nothing is copied
        if (rc == PDWT_OK) rc = pdwt_forward(p);
        if (rc != PDWT_OK) {
            v->state = PDWT_FORWARD_ERROR;
            return rc;
        }
    }
    v->state = PDWT_FORWARD;
    return PDWT_OK;
}

int pdwt_volume_inverse(pdwt_volume_handle v) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "W.inverse() has already been run. Inverse is available in W.get_image()");
    if (v->state == PDWT_FORWARD_ERROR || v->state == PDWT_THRESHOLD_ERROR || v->state == PDWT_CREATION_ERROR)
        return VFAIL(PDWT_ERR_STATE, "inverse transform not computed, as there was an error in a previous stage");
    DeviceGuard guard(v->device);
    for (int l = v->nlevels; l >= 1; l--) {
        pdwt_handle p = v->plans[l - 1];
        // band A's depth-low half was written in place: by the level below, by the forward or by set_coeff
        int rc = pdwt_set_coeff(p, reinterpret_cast<const real_t*>(pdwt_coeff_ptr(p, 0)), 0, 1);
        if (rc == PDWT_OK) rc = pdwt_inverse(p);
        if (rc == PDWT_OK) {
            const long long P = (long long)v->nr[l - 1] * v->nc[l - 1];
            const hipError_t e = launch_dwt3_depth_inv(stack_ptr(v, l), approx_ptr(v, l - 1), v->nz[l - 1], P, v->hlen, v->rec, v->seg_inv[l - 1], v->stream);
            if (e != hipSuccess) rc = VFAIL(PDWT_ERR_HIP, "depth synthesis of level %d failed: %s", l, hipGetErrorString(e));
        }
        if (rc != PDWT_OK) {
            v->state = PDWT_INVERSE_ERROR;
            return rc;
        }
    }
    v->state = PDWT_INVERSE;
    return PDWT_OK;
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
    PDWT_TRY(pdwt_copy(v->plans[0], dst, v->image, n, 2));
    return n;
}

int pdwt_volume_set_image(pdwt_volume_handle v, const pdwt_real* src, int mem_is_on_device) {
    if (!v || !src) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_image: null argument");
    DeviceGuard guard(v->device);
    const long long n = (long long)v->Nz * v->Nr * v->Nc;
    if (!(mem_is_on_device && src == v->image)) {
        PDWT_TRY(pdwt_copy(v->plans[0], v->image, src, n, mem_is_on_device ? 0 : 1));
        if (mem_is_on_device) HIP_TRY(hipStreamSynchronize(v->stream));  // like pdwt_set_image: the source may be reused at once
    }
    v->state = PDWT_INIT;
    return PDWT_OK;
}

long long pdwt_volume_coeff_count(pdwt_volume_handle v, int num, int* depth, int* rows, int* cols) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    SubBand s;
    if (!locate(v, num, &s)) return VFAIL(PDWT_ERR_ARG, "coefficient index %d out of range", num);
    if (depth) *depth = s.depth;
    if (rows) *rows = s.rows;
    if (cols) *cols = s.cols;
    return elems(s);
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
    PDWT_TRY(pdwt_copy(v->plans[s.level - 1], dst, sub_ptr(v, s), elems(s), 2));
    return elems(s);
}

int pdwt_volume_set_coeff(pdwt_volume_handle v, const pdwt_real* src, int num, int mem_is_on_device) {
    if (!v || !src) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_set_coeff: null argument");
    SubBand s;
    if (!locate(v, num, &s)) return VFAIL(PDWT_ERR_ARG, "coefficient index %d out of range", num);
    DeviceGuard guard(v->device);
    real_t* dst = sub_ptr(v, s);
    if (!(mem_is_on_device && src == dst)) {
        PDWT_TRY(pdwt_copy(v->plans[s.level - 1], dst, src, elems(s), mem_is_on_device ? 0 : 1));
        if (mem_is_on_device) HIP_TRY(hipStreamSynchronize(v->stream));
    }
    // as pdwt_set_coeff: once the approximation has been supplied again the coefficients are current
    if (num == 0 && v->state == PDWT_INVERSE) v->state = PDWT_FORWARD;
    return PDWT_OK;
}

intptr_t pdwt_volume_image_ptr(pdwt_volume_handle v) { return v ? (intptr_t)v->image : 0; }

intptr_t pdwt_volume_coeff_ptr(pdwt_volume_handle v, int num) {
    SubBand s;
    if (!v || !locate(v, num, &s)) return 0;
    DeviceGuard guard(v->device);
    return (intptr_t)sub_ptr(v, s);
}

int pdwt_volume_soft_threshold(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs, int normalize) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    return threshold_impl(v, EW_SOFT, beta, do_thresh_appcoeffs, normalize, "soft_threshold");
}

int pdwt_volume_hard_threshold(pdwt_volume_handle v, pdwt_real beta, int do_thresh_appcoeffs, int normalize) {
    if (!v) return VFAIL(PDWT_ERR_ARG, "null volume handle");
    return threshold_impl(v, EW_HARD, beta, do_thresh_appcoeffs, normalize, "hard_threshold");
}

int pdwt_volume_norms(pdwt_volume_handle v, double out[2]) {
    if (!v || !out) return VFAIL(PDWT_ERR_ARG, "pdwt_volume_norms: null argument");
    if (v->state == PDWT_INVERSE)
        return VFAIL(PDWT_ERR_STATE, "norms: the coefficients were modified by inverse()");
    DeviceGuard guard(v->device);
    const int L = v->nlevels;
    std::vector<std::vector<double>> sums(L);
    for (int l = 1; l <= L; l++) {
        pdwt_handle p = v->plans[l - 1];
        double* d_stats = nullptr;
        PDWT_TRY(pdwt_band_stats_async(p, nullptr));
        PDWT_TRY(pdwt_adaptive_slots(p, &d_stats, nullptr, nullptr));
        sums[l - 1].resize((size_t)4 * 2 * v->nz[l] * 2);
        HIP_TRY(hipMemcpyAsync(sums[l - 1].data(), d_stats, sums[l - 1].size() * sizeof(double), hipMemcpyDeviceToHost, v->stream));
    }
    HIP_TRY(hipStreamSynchronize(v->stream));
    // all details, and the depth-low half of band A at the last level only; [band][image][2], in a fixed order, in double
    double n1 = 0, n2 = 0;
    for (int l = 1; l <= L; l++) {
        const int half = v->nz[l], batch = 2 * half;
        for (int b = 0; b < 4; b++)
            for (int i = 0; i < batch; i++) {
                if (b == 0 && i < half && l != L) continue;
                n1 += sums[l - 1][((size_t)b * batch + i) * 2];
                n2 += sums[l - 1][((size_t)b * batch + i) * 2 + 1];
            }
    }
    out[0] = n1, out[1] = n2;
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

}  // extern "C"
#pragma GCC visibility pop
