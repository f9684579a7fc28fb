// volume.hpp -- host-side 3D transforms of a volume [Nz][Nr][Nc] (pdwt_volume_* of include/pypwt_amd.h).
//
// No reference counterpart: "3D is not handled at the moment" (pdwt/README.md:29), the constructor stops at
// "ndim=%d is not implemented" (pdwt/src/wt.cu:170-172).
//
// The C handle is a pdwt_volume: what both transforms keep, and the few operations the entry points of volume.cpp need from
// either.  The object behind it is a pdwt::VolumeDwt (pdwt_volume_create) or a pdwt::VolumeSwt (pdwt_volume_create_swt); each
// carries its own layout picture.
#pragma once

#include <vector>

#include "plan.hpp"
// the range and level tables of the volume's operators and their index math; the kernels belong to launch_volume_ops.hip
#define PDWT_INLINE_HELPERS_ONLY
#include "volume_ops_kernels.hpp"
#include "volume_shift_kernels.hpp"
#undef PDWT_INLINE_HELPERS_ONLY

namespace pdwt {

// Device workspace of the operators that pool slices and levels into the sub-bands of ONE volume (band_stats, estimate_sigma,
// threshold_bands, denoise, select_magnitude, keep_largest, norms_async): one block, allocated by the first of them that is called
// (volume.cpp: ensure_ops), as AdaptiveWs is for a plan.
struct VolumeWs {
    void* block = nullptr;
    double* stats = nullptr;                // [1 + 7 L][2]: sum |c|, sum c^2 of every sub-band
    double* sigma = nullptr;                // [1]
    double* norms = nullptr;                // [2]
    real_t* table = nullptr;                // [1 + 7 L] thresholds of the last denoise
    void* sel_state = nullptr;              // radix select of one image (select_kernels.hpp)
    unsigned* sel_hist = nullptr;
    long long* sp_k = nullptr;              // [1] each: K as the caller gave it, the selected key, the threshold, the kept count
    void* sp_key = nullptr;
    real_t* sp_threshold = nullptr;
    unsigned long long* sp_kept = nullptr;
    void* h_stage = nullptr;                // pinned: K, or a noise level, on its way to the device
    hipEvent_t staged = nullptr;
    VolLevels levels{};                     // the level plans' own slots
};

// one of the 1 + 7 L sub-bands of a volume
struct SubBand {
    int level, half, band;  // level 1 .. L, depth half (0 low, 1 high), band of that level's 2D transform (0 A, 1 H, 2 V, 3 D)
    int depth, rows, cols;
    long long elems() const { return (long long)depth * rows * cols; }
};

}  // namespace pdwt

struct pdwt_volume {
    int device = 0;
    hipStream_t stream = nullptr;
    int Nz = 0, Nr = 0, Nc = 0, nlevels = 0, hlen = 0;
    int state = PDWT_INIT;
    char wname[128] = {0};
    const int do_swt;                   // which of the two objects this is; read by pdwt_volume_is_swt and volume.cpp's as_dwt only
    real_t* image = nullptr;            // [Nz][Nr][Nc]
    std::vector<int> nz, nr, nc;        // [l]: sizes of A_l, [0] = the image
    std::vector<int> seg_fwd, seg_inv;  // [l - 1]: steps per depth segment of level l's depth passes
    std::vector<int> seg_fwd_chosen, seg_inv_chosen;  // [l - 1]: the chooser's values (pdwt_volume_set_depth_segments restores them)
    std::vector<int> width;             // [l - 1]: columns per thread of level l's depth passes (a stationary volume: of the analysis)
    pdwt::FilterBank dec{}, rec{};
    // the group operators (group_soft_threshold, group_norm): every level's members and pieces, fixed with the layout, and the
    // norm's workspace -- [0] the result slot, then one partial sum per piece --, allocated by the first call that needs it
    pdwt::VolGroupTable groups{};
    double* group_ws = nullptr;
    // cycle spinning (pdwt_volume_set_cycle_spinning): every forward shifts the image by a fresh draw of `rng`; `shift` is what the
    // image is shifted by IN ALL since the caller gave it (the draws of forwards in a row add up), undone by the next inverse
    int do_cycle_spinning = 0;
    int shift[3] = {0, 0, 0};
    unsigned long long rng = 0;
    // pdwt_volume_cycle_spin_async: one block of two volumes -- the kept source and the running mean --, allocated by its first call
    void* spin_block = nullptr;
    real_t *spin_src = nullptr, *spin_acc = nullptr;

    explicit pdwt_volume(int swt) : do_swt(swt) {}
    pdwt_volume(const pdwt_volume&) = delete;
    // releases what the object owns; the caller has selected `device`
    virtual ~pdwt_volume() = default;

    // the level loops of the two directions, without the state handling
    virtual int forward_levels() = 0;
    virtual int inverse_levels() = 0;
    virtual real_t* sub_ptr(const pdwt::SubBand& s) const = 0;
    virtual real_t* approx_ptr(int level) const = 0;  // A_l; the image for l = 0
    // at least one volume of scratch that is dead while the image is current: the level-1 stack
    virtual real_t* shift_scratch() const = 0;
    // host <-> device copies on the volume's stream (kind 0 d2d, 1 h2d, 2 d2h; the host kinds return when the copy is done)
    virtual int copy(void* dst, const void* src, long long count, int kind) = 0;
    // the global soft / hard threshold: level_betas[l - 1] on the details of level l, app_beta_or_nan on A_L (NaN: left alone)
    virtual int threshold(int op, const real_t* level_betas, real_t app_beta_or_nan, const char* what) = 0;
    virtual int norms(double out[2]) = 0;
    // what a sweep that writes the coefficients in place does first: the level plans of a decimated volume are told that their
    // coefficients are current, a stationary volume checks the sweeps' size limit
    virtual int enter_sweep(const char* what) = 0;
    // add_wavelet: c += alpha c_other on this volume's stream; `other` is the same kind of object with the same layout
    virtual int axpy(const pdwt_volume* other, real_t alpha) = 0;
    virtual int walk_steps(int level, bool inverse) const = 0;  // steps of a whole depth walk of that level
    // columns per thread of level l's depth pass in that direction (pdwt_volume_depth_width)
    virtual int depth_width(int level, bool /*inverse*/) const { return width[level - 1]; }
    // pdwt_volume_set_filters: the bank of every stage, or none of them where one refuses
    virtual int set_filters(int hlen, const real_t* dec_lo, const real_t* dec_hi, const real_t* rec_lo, const real_t* rec_hi);
};

namespace pdwt {

// The DECIMATED volume.  One level = the depth pass (dwt3_axis_kernels.hpp) followed by ONE level of the batched 2D transform on
// the stack of low and high slices it wrote.  A volume owns its image and one batched 2D plan per level (batch = 2 div2(Nz),
// levels = 1):
//
//   image [Nz][Nr][Nc]
//   level l:  plan_l's image slot  = the stack [2 div2(Nz_{l-1})][Nr_{l-1}][Nc_{l-1}] the depth pass writes
//             plan_l's bands A,H,V,D, each [batch][div2 Nr][div2 Nc]: the first half of the images of a band is its depth-low
//             sub-band, the second half its depth-high one -- the eight 3D sub-bands are views, nothing is copied.
//             The depth-low half of band A is A_l: the next level's depth pass reads it in place; for l < L it is an
//             intermediate, for l = L the coefficient num 0.
//
// Footprint: about 3.3 volumes -- the image, and per level a stack plus a coefficient region of that level's size
// (1 + 2 (1 + 1/8 + 1/64 + ...)).  Not shaved here.
struct VolumeDwt final : pdwt_volume {
    std::vector<pdwt_handle> plans;  // [l - 1]: the batched 2D plan of level l; plans[0] owns the stream unless the caller gave one
    // the swept ranges of the K-term operators, fixed with the layout: pieces of the histogram passes (1024 threads) and of the keep sweep
    VolRangeTable rt_hist{}, rt_keep{};
    unsigned long long n_details = 0, n_app = 0;  // elements of the 7 L detail sub-bands, of A_L
    VolumeWs* ops = nullptr;

    VolumeDwt() : pdwt_volume(0) {}
    ~VolumeDwt() override;
    int forward_levels() override;
    int inverse_levels() override;
    real_t* sub_ptr(const SubBand& s) const override;
    real_t* approx_ptr(int level) const override;
    int copy(void* dst, const void* src, long long count, int kind) override;
    int threshold(int op, const real_t* level_betas, real_t app_beta_or_nan, const char* what) override;
    int norms(double out[2]) override;
    int enter_sweep(const char* what) override;
    int axpy(const pdwt_volume* other, real_t alpha) override;
    int walk_steps(int level, bool inverse) const override;
    int set_filters(int hlen, const real_t* dec_lo, const real_t* dec_hi, const real_t* rec_lo, const real_t* rec_hi) override;
    real_t* stack_ptr(int level) const;  // what level l's depth pass writes: its plan's image slot
    real_t* shift_scratch() const override { return stack_ptr(1); }
};

// The STATIONARY volume: no level plans, ONE device block.  Level l = the a-trous depth pass (swt3_axis_kernels.hpp)
// A_{l-1} -> stack at dilation f = 2^(l-1), then one batched 2D SWT level (launch.hpp: Swt2DArgs{f, bstride = P}, batch 2 Nz)
// stack -> the level's four band arrays, each [2 Nz][P]: the first half of an array is the depth-low sub-band, the second half the
// depth-high one (A = aaa | daa, H = ada | dda, V = aad | dad, D = add | ddd: volume.cpp, kSub).  aaa of level l is A_l: the next
// level's depth pass reads it in place; for l < L an intermediate, for l = L coefficient 0.
//
//   block = image [Nz][P] | stack [2 Nz][P] | level 1: A H V D | ... | level L: A H V D | sums, partial sums, thresholds | slack
//
// Footprint: (3 + 8 L) volumes (1 + 2 + 4 x 2 per level) plus 256-B alignment of every buffer, the few KiB of the operators'
// sums and at least 16 B of slack behind everything a 2D kernel may address (the one-launch 2D kernels may read up to 12 B
// past the last plane).  Not shaved here.  nz / nr / nc hold (Nz, Nr, Nc) at every level: every band has the image's shape.
struct VolumeSwt final : pdwt_volume {
    bool own_stream = false;
    void* block = nullptr;            // `image` points at its start
    real_t* stack = nullptr;
    std::vector<real_t*> band;        // [4 (l - 1) + b]: band array b (0 A, 1 H, 2 V, 3 D) of level l
    std::vector<int> width_inv;       // [l - 1]: columns per thread of level l's depth synthesis (the forward's is `width`)
    std::vector<BandTable> bt;        // [l - 1]: the four arrays of level l as 4 bands x 2 "images" (the depth halves) of Nz P values
    double* stats = nullptr;          // [L][4][2][2]
    double* partial = nullptr;        // [L][2 * pieces of a level]
    real_t* table = nullptr;          // [L][4][2] thresholds of the last sweep
    int pieces = 0;                   // workgroups of one level's sweep
    real_t* h_table = nullptr;        // pinned: the thresholds on their way to the device
    hipEvent_t staged = nullptr;      // ... have left it

    VolumeSwt() : pdwt_volume(1) {}
    ~VolumeSwt() override;
    int forward_levels() override;
    int inverse_levels() override;
    real_t* sub_ptr(const SubBand& s) const override;
    real_t* approx_ptr(int level) const override;
    real_t* shift_scratch() const override { return stack; }
    int copy(void* dst, const void* src, long long count, int kind) override;
    int threshold(int op, const real_t* level_betas, real_t app_beta_or_nan, const char* what) override;
    int norms(double out[2]) override;
    int enter_sweep(const char* what) override;
    int axpy(const pdwt_volume* other, real_t alpha) override;
    int walk_steps(int level, bool inverse) const override;
    int depth_width(int level, bool inverse) const override { return (inverse ? width_inv : width)[level - 1]; }
    Swt2DArgs level_args(int level, bool inverse) const;
    int ops_check(const char* what) const;  // the sweeps' limit of 2^31 - 1 values per sub-band
};

}  // namespace pdwt
