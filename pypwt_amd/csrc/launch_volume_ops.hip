// launch_volume_ops.hip -- launchers of the per-sub-band and K-term operators of a volume (gfx950).
#include "launch.hpp"
#include "launch_util.hpp"
// sweep_range and the select's digit logic without a second definition of the kernels of launch_ops.hip
#define PDWT_INLINE_HELPERS_ONLY
#include "select_kernels.hpp"
#undef PDWT_INLINE_HELPERS_ONLY
#include "volume_ops_kernels.hpp"
#include "volume_shift_kernels.hpp"

namespace pdwt {

static int vol_blocks(const VolRangeTable& t, int with_app) {
    if (t.nranges < 2 || t.nranges > kVolMaxRanges) return 0;
    return t.blk[with_app ? t.nranges : t.nranges - 1];
}

hipError_t launch_vol_select_hist(const VolRangeTable& t, int with_app, int pass, const long long* d_k, unsigned long long n, const void* state,
                                  unsigned* hist, hipStream_t s) {
    const int blocks = vol_blocks(t, with_app);
    if (blocks < 1 || pass < 0 || pass >= kSelectPasses) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_select_hist_kernel, dim3(blocks), dim3(kSelectHistThreads), 0, s, t, pass, d_k, n, static_cast<const SelectState*>(state),
                       hist);
    return hipGetLastError();
}

hipError_t launch_vol_keep(const VolRangeTable& t, int with_app, const void* d_key, hipStream_t s) {
    const int blocks = vol_blocks(t, with_app);
    if (blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_keep_kernel, dim3(blocks), dim3(kVolKeepThreads), 0, s, t, static_cast<const select_key_t*>(d_key));
    return hipGetLastError();
}

hipError_t launch_vol_stats_reduce(const VolLevels& v, double* stats, hipStream_t s) {
    if (v.nlevels < 1 || v.nlevels > kVolMaxLevels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_stats_reduce_kernel, dim3(1 + 7 * v.nlevels), dim3(64), 0, s, v, stats);
    return hipGetLastError();
}

hipError_t launch_vol_norms(const double* stats, int nbands, double* out2, hipStream_t s) {
    hipLaunchKernelGGL(vol_norms_kernel, dim3(1), dim3(64), 0, s, stats, nbands, out2);
    return hipGetLastError();
}

hipError_t launch_vol_table(const VolLevels& v, const double* stats, const double* sigma, int method, double visu, real_t* d_table, hipStream_t s) {
    if (v.nlevels < 1 || v.nlevels > kVolMaxLevels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_table_kernel, dim3(cdiv(1 + 7 * v.nlevels, 64)), dim3(64), 0, s, v, stats, sigma, method, visu, d_table);
    return hipGetLastError();
}

hipError_t launch_vol_expand(const VolLevels& v, const real_t* d_table, hipStream_t s) {
    if (v.nlevels < 1 || v.nlevels > kVolMaxLevels || v.entry[v.nlevels] < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_expand_kernel, dim3(cdiv(v.entry[v.nlevels], 256)), dim3(256), 0, s, v, d_table);
    return hipGetLastError();
}

static int vol_group_blocks(const VolGroupTable& t) {
    if (t.nlevels < 1 || t.nlevels > kVolMaxLevels || t.chunk < 4 || (t.chunk & 3)) return 0;
    return t.blk[t.nlevels];
}

hipError_t launch_vol_group_soft(const VolGroupTable& t, const VolGroupBetas& betas, int with_app, hipStream_t s) {
    const int blocks = vol_group_blocks(t);
    if (blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_group_soft_kernel, dim3(blocks), dim3(kVolGroupThreads), 0, s, t, betas, with_app ? 1 : 0);
    return hipGetLastError();
}

// partial: one double per workgroup (vol_group_partials of them); out: where the sum goes (device memory)
hipError_t launch_vol_group_norm(const VolGroupTable& t, int with_app, double* partial, double* out, hipStream_t s) {
    const int blocks = vol_group_blocks(t);
    if (blocks < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vol_group_norm_kernel, dim3(blocks), dim3(kVolGroupThreads), 0, s, t, with_app ? 1 : 0, partial);
    hipLaunchKernelGGL(vol_group_norm_final_kernel, dim3(1), dim3(64), 0, s, partial, blocks, out);
    return hipGetLastError();
}

// out = circshift(in, sz, sr, sc) on [Nz][Nr][Nc], the shifts of any sign and size; in and out must not overlap
hipError_t launch_vol_circshift(const real_t* in, real_t* out, int Nz, int Nr, int Nc, int sz, int sr, int sc, hipStream_t s) {
    if (Nz < 1 || Nr < 1 || Nc < 1 || !in || !out || in == out) return hipErrorInvalidValue;
    const VolShiftGeom g = vol_shift_geom_of(Nz, Nr, Nc, sz, sr, sc, false, in, out);
    const dim3 grid(vol_shift_grid(g)), block(kVolShiftThreads);
    if (g.mode == 2) hipLaunchKernelGGL(vol_circshift_kernel<2>, grid, block, 0, s, in, out, g);
    else if (g.mode == 1) hipLaunchKernelGGL(vol_circshift_kernel<1>, grid, block, 0, s, in, out, g);
    else hipLaunchKernelGGL(vol_circshift_kernel<0>, grid, block, 0, s, in, out, g);
    return hipGetLastError();
}

// acc = (first ? 0 : acc) + w circshift(rec, -sz, -sr, -sc): the shift (sz, sr, sc) that was applied is undone
hipError_t launch_vol_unshift_acc(const real_t* rec, real_t* acc, int Nz, int Nr, int Nc, int sz, int sr, int sc, real_t w, int first, hipStream_t s) {
    if (Nz < 1 || Nr < 1 || Nc < 1 || !rec || !acc || rec == acc) return hipErrorInvalidValue;
    const VolShiftGeom g = vol_shift_geom_of(Nz, Nr, Nc, sz, sr, sc, true, rec, acc);
    const dim3 grid(vol_shift_grid(g)), block(kVolShiftThreads);
    const int f = first ? 1 : 0;
    if (g.mode == 2) hipLaunchKernelGGL(vol_unshift_acc_kernel<2>, grid, block, 0, s, rec, acc, g, w, f);
    else if (g.mode == 1) hipLaunchKernelGGL(vol_unshift_acc_kernel<1>, grid, block, 0, s, rec, acc, g, w, f);
    else hipLaunchKernelGGL(vol_unshift_acc_kernel<0>, grid, block, 0, s, rec, acc, g, w, f);
    return hipGetLastError();
}

}  // namespace pdwt
