// volume.hpp -- host-side 3D DWT of a volume [Nz][Nr][Nc] (pdwt_volume_* of include/pypwt_amd.h).
//
// No reference counterpart: "3D is not handled at the moment" (pdwt/README.md:29), the constructor stops at
// "ndim=%d is not implemented" (pdwt/src/wt.cu:170-172).
//
// One level = the depth pass (dwt3_axis_kernels.hpp) followed by ONE level of the batched 2D transform on the stack of low and
// high slices it wrote.  A volume owns its image and one batched 2D plan per level (batch = 2 div2(Nz_l), levels = 1):
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
//
// The STATIONARY volume (do_swt: pdwt_volume_create_swt) is the same handle without level plans: one device block of (3 + 8 L)
// volumes; its fields and layout are at the end of struct pdwt_volume.
#pragma once

#include <vector>

#include "plan.hpp"
// the range and level tables of the volume's operators and their index math; the kernels belong to launch_volume_ops.hip
#define PDWT_INLINE_HELPERS_ONLY
#include "volume_ops_kernels.hpp"
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

}  // namespace pdwt

struct pdwt_volume {
    int device = 0;
    hipStream_t stream = nullptr;
    int Nz = 0, Nr = 0, Nc = 0, nlevels = 0, hlen = 0;
    int state = PDWT_INIT;
    char wname[128] = {0};
    real_t* image = nullptr;            // [Nz][Nr][Nc], owned
    std::vector<pdwt_handle> plans;     // [l - 1]: the batched 2D plan of level l; plans[0] owns the stream unless the caller gave one
    std::vector<int> nz, nr, nc;        // [l]: sizes of A_l, [0] = the image
    std::vector<int> seg_fwd, seg_inv;  // [l - 1]: steps per depth segment of level l's depth passes
    std::vector<int> seg_fwd_chosen, seg_inv_chosen;  // [l - 1]: the chooser's values (pdwt_volume_set_depth_segments restores them)
    std::vector<int> width;             // [l - 1]: columns per thread of level l's depth passes
    pdwt::FilterBank dec{}, rec{};
    // the swept ranges of the K-term operators, fixed with the layout: pieces of the histogram passes (1024 threads) and of the keep sweep
    pdwt::VolRangeTable rt_hist{}, rt_keep{};
    unsigned long long n_details = 0, n_app = 0;  // elements of the 7 L detail sub-bands, of A_L
    pdwt::VolumeWs* ops = nullptr;

    // ---- the stationary volume (do_swt, pdwt_volume_create_swt): no level plans, ONE device block.  Level l = the a-trous depth
    // pass (swt3_axis_kernels.hpp) A_{l-1} -> stack at dilation f = 2^(l-1), then one batched 2D SWT level (launch.hpp:
    // Swt2DArgs{f, bstride = P}, batch 2 Nz) stack -> the level's four band arrays, each [2 Nz][P]: the first half of an array is
    // the depth-low sub-band, the second half the depth-high one (A = aaa | daa, H = ada | dda, V = aad | dad, D = add | ddd: kSub).
    // aaa of level l is A_l: the next level's depth pass reads it in place; for l < L an intermediate, for l = L coefficient 0.
    //
    //   block = image [Nz][P] | stack [2 Nz][P] | level 1: A H V D | ... | level L: A H V D | sums, partial sums, thresholds | slack
    //
    // Footprint: (3 + 8 L) volumes (1 + 2 + 4 x 2 per level) plus 256-B alignment of every buffer, the few KiB of the operators'
    // sums and at least 16 B of slack behind everything a 2D kernel may address (the one-launch 2D kernels may read up to 12 B
    // past the last plane).  Not shaved here.  nz / nr / nc hold (Nz, Nr, Nc) at every level: every band has the image's shape.
    int do_swt = 0;
    bool own_stream = false;
    void* swt_block = nullptr;
    real_t* swt_stack = nullptr;
    std::vector<real_t*> swt_band;        // [4 (l - 1) + b]: band array b (0 A, 1 H, 2 V, 3 D) of level l
    std::vector<int> width_inv;           // [l - 1]: columns per thread of level l's depth synthesis (the forward's is `width`)
    std::vector<pdwt::BandTable> swt_bt;  // [l - 1]: the four arrays of level l as 4 bands x 2 "images" (the depth halves) of Nz P values
    double* swt_stats = nullptr;          // [L][4][2][2]
    double* swt_partial = nullptr;        // [L][2 * pieces of a level]
    real_t* swt_table = nullptr;          // [L][4][2] thresholds of the last sweep
    int swt_pieces = 0;                   // workgroups of one level's sweep
    real_t* swt_h_table = nullptr;        // pinned: the thresholds on their way to the device
    hipEvent_t swt_staged = nullptr;      // ... have left it
};
