// lazy_state.hpp -- what every entry point of the C ABI owes a plan's deferred soft threshold.
//
// The table of docs/KERNELS.md ("The lazy state of a plan: what every entry point owes") as code: plan.cpp's settle() performs a
// row, tests/test_plan_model_cpu.py holds it against tests/plan_model.py.  Plain C++17, no HIP: the CPU tests read it too.
//
// Two slots, never merged: `pending` (requested, the fused inverse will apply it) and `consumed` (an inverse applied it on the fly,
// the stored details still lack it).  Both can be live at once: a failed un-shift leaves `consumed` set with state
// PDWT_INVERSE_ERROR, where nothing refuses and a new soft_threshold defers.
#pragma once

namespace pdwt {

enum class Entry {
    forward,
    inverse,
    soft,             // soft_threshold, soft_threshold_norms
    eager_threshold,  // hard_threshold, group_soft_threshold, shrink, proj_linf
    norms,            // norm1, norm2sq, norms_async
    read_stats,       // band_stats_async, estimate_sigma_async, select_magnitude_async
    band_sweep,       // threshold_bands, denoise_async, keep_largest_async
    add_wavelet,      // both operands
    get_coeff,        // get_coeff, get_coeff_at, get_coeff_region
    coeff_ptr,
    set_coeff,
    set_image,
    clone,
    untouched,  // get_image, get_image_at, circshift, set_filters_*, adaptive_slots, ...
    count_
};

enum class Pending { keep, apply, drop, consume };  // consume: the inverse applies it on the fly and it becomes `consumed`
enum class Consumed { keep, write_back, drop };

struct LazyRow {
    bool refuses_after_inverse;  // turned down in state PDWT_INVERSE, before anything is touched
    Pending pending;
    Consumed consumed;  // `keep` where the refusal covers it: a consumed threshold outside PDWT_INVERSE stays owed
};

constexpr LazyRow lazy_row(Entry e) {
    switch (e) {
        case Entry::forward: return {false, Pending::drop, Consumed::drop};  // the coefficients they meant are overwritten
        case Entry::inverse: return {true, Pending::consume, Consumed::keep};
        case Entry::soft: return {true, Pending::apply, Consumed::keep};  // the earlier one first; the new one may become pending
        case Entry::eager_threshold: return {true, Pending::apply, Consumed::keep};
        case Entry::norms: return {false, Pending::apply, Consumed::write_back};
        case Entry::read_stats: return {false, Pending::apply, Consumed::write_back};
        case Entry::band_sweep: return {true, Pending::apply, Consumed::keep};
        case Entry::add_wavelet: return {true, Pending::apply, Consumed::keep};
        case Entry::get_coeff: return {true, Pending::apply, Consumed::keep};
        case Entry::coeff_ptr: return {false, Pending::apply, Consumed::write_back};
        case Entry::set_coeff: return {false, Pending::apply, Consumed::write_back};  // it meant the old contents
        case Entry::set_image: return {false, Pending::keep, Consumed::write_back};  // the getters are legal again in PDWT_INIT
        case Entry::clone: return {false, Pending::apply, Consumed::write_back};
        default: return {false, Pending::keep, Consumed::keep};
    }
}

}  // namespace pdwt
